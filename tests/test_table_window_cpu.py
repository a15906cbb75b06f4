"""The table executor's window arithmetic (fantoch_amd/csrc/table_window.h, the
code the kernels of table_exec.hip run on a voter's lane) compiled for the
host under AddressSanitizer and UBSan and driven as a stand-alone program
(tests/table_window_main.cpp) with more than 200,000 ranges per form, every
answer compared with the restatement's EventSet.  CPU only."""
import os
import random
import shutil
import subprocess
import tempfile

import pytest

from table_ref import FX_ERR_VOTE_RANGE, EventSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or "g++"
FX_ERR_CAPACITY = 2
TOP = (1 << 32) - 1
# form -> (window, a range that starts at the frontier may end beyond the window)
FORMS = {"word": (32, False), "word_aligned": (32, True), "ring": (2048, True), "ring_unrolled": (2048, True)}
BASES = [0, 2048 - 40, 2048 + 40, 2 * 2048 - 40, 2 * 2048 + 40, 5 * 2048 - 40]
HIGH = (1 << 32) - 3000


@pytest.fixture(scope="module")
def program():
    if shutil.which(CXX) is None:
        pytest.skip("needs a host C++ compiler (%s)" % CXX)
    d = tempfile.mkdtemp()
    try:
        probe = os.path.join(d, "probe.cpp")
        open(probe, "w").write("int main() { return 0; }\n")
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        ok = subprocess.run([CXX] + san + ["-o", os.path.join(d, "probe"), probe], capture_output=True)
        if ok.returncode != 0 or subprocess.run([os.path.join(d, "probe")], capture_output=True).returncode != 0:
            pytest.skip("%s has no AddressSanitizer / UBSan runtime" % CXX)
        exe = os.path.join(d, "table_window_main")
        subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + san +
                       ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "fantoch_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tests", "table_window_main.cpp")],
                       check=True, capture_output=True, text=True)
        yield exe
    finally:
        shutil.rmtree(d, ignore_errors=True)


def gappy_range(rng, f, win):
    """As tests/table_edges.py gappy: an end within the window (exactly at its
    end one time in 16, up to 3 beyond it one time in 16), a start up to 100
    below; one time in 8 a start at or below the frontier + 1 instead."""
    d = rng.randrange(16)
    end = f + (win if d == 0 else win + 1 + rng.randrange(3) if d == 1 else 1 + rng.randrange(win))
    start = end - rng.randrange(101)
    if rng.randrange(8) == 0:
        start = f + 1 - rng.randrange(4)
    return start, end


def random_range(rng, f, win):
    """Ends from 10 below the frontier to 40 beyond the window; starts next to
    the end, next to the frontier, anywhere in between, or 1; one time in 200
    a range from the frontier far beyond the window."""
    if rng.randrange(200) == 0:
        return f + 1, f + win + 1 + rng.randrange(10000)
    end = f - 10 + rng.randrange(win + 51)
    how = rng.randrange(10)
    if how < 5:
        start = end - rng.randrange(5)
    elif how < 8:
        start = f - 1 + rng.randrange(4)
    elif how == 8:
        start = end - rng.randrange(win + 50)
    else:
        start = 1
    return start, end


def expected(es, win, aligned, start, end):
    """The kernel's rule per tier over the restatement's EventSet: a range
    whose end lies beyond the window is FX_ERR_CAPACITY unless the tier takes
    ranges that start at the frontier and this one does."""
    if end <= es.frontier:
        return FX_ERR_VOTE_RANGE
    if end - es.frontier > win and not (aligned and start <= es.frontier + 1):
        return FX_ERR_CAPACITY
    return 0 if es.add_range(start, end) else FX_ERR_VOTE_RANGE


def drive(program, form, base, style, seed, count):
    """One run of the program from frontier `base`; returns the statuses seen."""
    win, aligned = FORMS[form]
    rng = random.Random(seed)
    es = EventSet()
    es.frontier = base
    lines, want = [], []
    for _ in range(count):
        start, end = style(rng, es.frontier, win)
        end = min(max(end, 1), TOP)
        start = min(max(start, 1), end)
        status = expected(es, win, aligned, start, end)
        lines.append("%d %d" % (start, end))
        want.append("%d %d %d" % (status, es.frontier, len(es.above)))
    run = subprocess.run([program, form, str(base)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, (form, base, seed, run.stderr[-2000:])
    got = run.stdout.split("\n")[:-1]
    assert len(got) == count
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s from %d, seed %d, range %d (%s): got %s, want %s" % (form, base, seed, i, lines[i], g, w)
    return [int(w.split()[0]) for w in want], es.frontier


@pytest.mark.parametrize("form", sorted(FORMS))
def test_window_arithmetic_against_the_event_set(program, form):
    total, seen, tops = 0, set(), 0
    for b, base in enumerate(BASES):
        for s, style in enumerate((gappy_range, random_range)):
            for rep in range(2):
                st, front = drive(program, form, base, style, 1000 * b + 10 * s + rep, 8500)
                assert front > base + 4 * FORMS[form][0]  # the frontier went round the ring more than once
                total += len(st)
                seen.update(st)
    for rep in range(40):  # short runs below 2**32: the frontier ends at or near the highest clock
        st, front = drive(program, form, HIGH, (gappy_range, random_range)[rep & 1], 7000 + rep, 300)
        total += len(st)
        tops += front == TOP
    assert total >= 200000 and seen == {0, FX_ERR_VOTE_RANGE, FX_ERR_CAPACITY}
    assert tops > 0
