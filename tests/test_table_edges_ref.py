"""What the restatements (tests/table_ref*.py) say of the edge streams of
tests/table_edges.py: the conditions that make them edge streams -- the ring
wraps, ranges overlap, capacities are met exactly -- hold on the CPU, so the
GPU tests (tests/test_table_edges_gpu.py) compare streams that are what they
claim to be.  CPU only."""
import random

import pytest

from fantoch_amd import table as ft

import table_edges as E
import table_ref as R
import table_ref_mk as RM
import table_ref_ps as RP
import table_shapes as T
import table_shapes_mk as TM
import table_shapes_ps as TP

TOP = (1 << 32) - 1
N_ENDS = [(16, 11, 9), (16, 16, 16), (16, 2, 1), (1, 1, 1), (2, 2, 1)]  # (n, fast quorum, stability threshold)


class NaiveSet:
    """EventSet.add_range as it was: one step per vote of the range."""

    def __init__(self):
        self.frontier, self.above = 0, set()

    def add_range(self, start, end):
        new = [v for v in range(max(start, self.frontier + 1), end + 1) if v not in self.above]
        self.above.update(new)
        while self.frontier + 1 in self.above:
            self.frontier += 1
            self.above.remove(self.frontier)
        return bool(new)


def test_event_set_costs_the_new_votes_and_answers_as_before():
    rng = random.Random(5)
    for _ in range(20):
        a, b = R.EventSet(), NaiveSet()
        for _ in range(400):
            end = max(1, a.frontier - 5 + rng.randrange(120))
            start = rng.choice([1, max(1, a.frontier), a.frontier + 1, a.frontier + 2, max(1, end - rng.randrange(40))])
            start = min(start, end)
            assert a.add_range(start, end) == b.add_range(start, end)
            assert (a.frontier, a.above) == (b.frontier, b.above)
    far = R.EventSet()
    assert far.add_range(7, 9) and far.add_range(1, TOP) and (far.frontier, far.above) == (TOP, set())
    assert not far.add_range(TOP, TOP)


@pytest.mark.parametrize("B,chunk,above", [(2028, 2048, 2028), (3 * 2048 - 20, 2048, 2048), (5000, None, 5000)])
def test_lift_single_key(B, chunk, above):
    thr = T.quorum_sizes(5, 1, False)[2]
    for st, ref in list(zip(T.generated(5, 1, False, 50), T.generated_ref(5, 1, False, 50)))[:8]:
        up, pre = E.lift(list(st), B, 5, T.KEYS, chunk)
        got = R.run_stream(up, 5, thr, T.KEYS)
        want = E.lifted_ref(ref, B, pre)
        assert got["err"] == 0 and got["max_above"] == above and got["max_pending"] == ref["max_pending"]
        for field in ("order", "release", "nexec", "stable"):
            assert got[field] == want[field], field
        assert got["steps"] == [[]] * pre + [[a + pre for a in step] for step in ref["steps"]]


def test_lift_to_the_highest_clock():
    """chunk=None costs the restatement one step per (key, voter), whatever B."""
    thr = T.quorum_sizes(5, 1, False)[2]
    for st, ref in list(zip(T.generated(5, 1, False, 50), T.generated_ref(5, 1, False, 50)))[:4]:
        B = TOP - E.highest(st)
        up, pre = E.lift(list(st), B, 5, T.KEYS)
        assert pre == 5 * T.KEYS and E.highest(up) == TOP
        got = R.run_stream(up, 5, thr, T.KEYS)
        want = E.lifted_ref(ref, B, pre)
        assert got["err"] == 0 and max(got["stable"]) == TOP
        assert all(got[f] == want[f] for f in ("order", "release", "nexec", "stable"))


@pytest.mark.parametrize("B,chunk", [(2028, 2048), (3 * 2048 - 20, 2048), (None, None)])
def test_lift_multi_key_and_shards(B, chunk):
    thr = T.quorum_sizes(5, 1, False)[2]
    mk = list(zip(TM.generated(5, 1, False, 2, 50), TM.generated_ref(5, 1, False, 2, 50)))[:4]
    sts, _, refs = TP.generated(2, 5, 1, 10)[0]
    for run, keys, pairs in ((RM.run_stream, TM.KEYS, mk), (RP.run_stream, TP.KEYS, list(zip(sts, refs)))):
        for st, ref in pairs:
            b = TOP - E.highest(st) if B is None else B
            up, pre = E.lift(list(st), b, 5, keys, chunk)
            got = run(up, 5, thr, keys)
            want = E.lifted_ref(ref, b, pre)
            assert got["err"] == 0 and got["max_gap_above"] == ref["max_gap_above"]
            assert all(got[f] == want[f] for f in ("order", "release", "nexec", "stable", "max_live", "max_stack"))
            if "sent" in ref:
                assert got["sent"] == want["sent"] and len(ref["sent"]) > 10


@pytest.mark.parametrize("win,events", [(2048, 1500), (32, 600)])
def test_gappy(win, events):
    for seed in range(8):
        st = E.gappy(seed, 3, 2, events, win)
        assert st == E.gappy(seed, 3, 2, events, win) and len(st) == events
        ref = R.run_stream(st, 3, 2, 2)
        assert ref["err"] == 0 and ref["max_above"] == win
        assert max(ref["stable"]) > 2 * win  # the ring went round more than twice
        partly, total = E.partly_seen(st, 3, 2)
        assert total == events and 3 * partly >= total
        assert ref["nexec"] > events // 10
        if win == 32:  # these stay on chip
            assert ref["max_pending"] <= 64
        else:
            assert ref["max_pending"] <= 512


@pytest.mark.parametrize("P", [64, 65, 512, 513])
def test_mass(P):
    st = E.mass(P, 3)
    ref = R.run_stream(st, 3, 2, 1)
    assert ref["err"] == 0 and ref["max_pending"] == P and ref["nexec"] == P
    assert [len(s) for s in ref["steps"]] == [0] * (P + 1) + [P, 0]
    ids = [(st[a][3], st[a][2]) for a in ref["order"]]
    assert ids == sorted(ids) and len({c for c, _ in ids}) == 7
    assert ref["order"] != sorted(ref["order"])  # arrival order is not the (clock, dot) order
    mk = RM.run_stream(st, 3, 2, 1)
    assert mk["order"] == ref["order"] and mk["max_live"] == P


@pytest.mark.parametrize("F,W", [(37, 32), (2 * 2048 - 5, 2048), (3 * 2048 + 31, 2048)])
@pytest.mark.parametrize("over", [0, 1])
def test_window_edge(F, W, over):
    st, gap = E.window_edge(F, W, over)
    assert st[gap] == ("D", 0, [(1, F + W + over, F + W + over)]) and st[gap - 1][0] == "A"
    ref = R.run_stream(st, 3, 2, 1)
    assert ref["err"] == 0 and ref["max_above"] == W + over and ref["max_pending"] == 1
    assert ref["order"] == [gap - 1] and ref["stable"] == [F + W + over]
    assert ref["release"][gap - 1] > gap + 2  # the op waits for a second voter
    # after F + 1 arrives voter 1's frontier has crossed the whole window
    table = R.VotesTable(3, 2)
    for ev in st[:gap + 3]:
        table.add_votes(ev[-1])
    assert table.clock[1].frontier == (F + W if over == 0 else F + W - 1)
    before = R.VotesTable(3, 2)
    for ev in st[:gap + 2]:
        before.add_votes(ev[-1])
    assert before.clock[1].frontier == F and len(before.clock[1].above) == W - 1  # all but F + 1 (and F + W)


@pytest.mark.parametrize("F,W", [(37, 32), (2 * 2048 - 5, 2048)])
def test_seen_inside(F, W):
    for st in E.seen_inside(F, W):
        ref = R.run_stream(st, 3, 2, 1)
        assert ref["err"] == R.FX_ERR_VOTE_RANGE and ref["nexec"] == 1 and ref["stable"] == [1]
        assert ref["max_above"] <= W and len(ref["steps"]) == len(st) - 1  # it stops at its last event
    ok = E.seen_inside(F, W)[0][:-1]  # the partly seen range is legal
    assert R.run_stream(ok, 3, 2, 1)["err"] == 0 and E.partly_seen(ok[1:], 3, 1)[0] >= 1


@pytest.mark.parametrize("n,fq,thr", N_ENDS)
def test_n_at_its_ends(n, fq, thr):
    vmax = 0
    for seed in range(8):
        st = ft.synth_table_streams(seed, n, fq, 8, 40, 50, 6, 4)
        ref = R.run_stream(st, n, thr, 8)
        assert ref["err"] == 0 and ref["nexec"] == 40
        assert ref["max_above"] <= 32 and ref["max_pending"] <= 64  # the on-chip tier holds them
        vmax = max([vmax] + [len(ev[-1]) for ev in st])
    assert vmax == fq


def test_max_votes_event():
    good, bad = E.max_votes_event(), E.max_votes_event(repeat=True)
    assert len(good[0][4]) == len(bad[0][4]) == 64
    ref = R.run_stream(good, 16, 16, 1, vmax=64)
    assert ref["err"] == 0 and ref["order"] == [0] and ref["stable"] == [2] and ref["max_above"] == 12
    ref = R.run_stream(bad, 16, 16, 1, vmax=64)
    assert ref["err"] == R.FX_ERR_VOTE_RANGE and ref["nexec"] == 0 and ref["stable"] == [0]
