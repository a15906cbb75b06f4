"""How an instance of the all-on-chip simulator (k_sim) ends when it fails
inside the handler loop (Sim::run_handlers_), the executor's search loop or
the event loop: those loops leave through their condition only, a failed step
skips the rest of its iteration by predicate, and what a failed instance
leaves behind must not depend on that shape.

EPaxos n = 5 f = 2, one client per region, 30 commands per client, 100 %
conflicts.  The failures:

  pool_fixed  the europe-west regions with one far replica (Sydney), default
              tables: the message pool (80 entries) overflows in send_batch,
              on the compiled-in build and on the run-time build
  pool_ring   the GCP5 regions with `ring_entries` one below the smallest pool
              the run gets through (found by bisection between 4 entries and
              the default geometry's: the oracle reports no peak of messages
              in flight), run-time build
  dots        GCP5 with `dot_slots` one below the smallest table the run gets
              through (bisection between 2 and 64): the dot table overflows
              in h_submit
  xslots      a synthetic planet (written under tmp_path): five regions 1 ms
              apart, except that the last is 500 ms from the first.  Every
              command conflicts, so whatever the last process commits waits
              there for the first process's commands, and its executor
              outgrows the 12 pending slots a process has on the compiled-in
              build (insert_vertex).  6 commands per client here: the rerun
              tier's executors hold 64 pending vertices, 30 commands in all
              stay below that
  events      GCP5 with max_events = 500: FX_ERR_SIM_EVENTS, both builds

For each: the status code; for the capacity failures the error site is a
`fail_cap(__LINE__)` line of the function the case is about (send_batch_,
h_submit, insert_vertex: read from the kernel's source), so the first
failure's and not a later one's; the event limit records no site; two runs
give identical outputs; the failing
instance gives the same rows alone and in the middle of a launch of passing
instances (one command per client, the same tables); those neighbours equal
the simulator oracle, and their rows, which flank the failing instance's rows
in the execution log, the latency log and the dot -> client table, are word
for word what a launch without the failing instance writes (the rows' unused
tails included: nothing was stored across a row boundary).  Through
fx_sim_run_tiered the capacity cases end equal to the oracle, histograms
included: the partial samples of the failed first attempt are subtracted
exactly.
"""
import os
import re

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import sim as S
from oracle import oracle_lib as O
from test_sim_gpu import assert_instance_parity, planet, to_oracle
from test_sim_percmd_paths import hists_vs_oracle, same_buffers

FAR = ["europe-west1", "europe-west2", "europe-west3", "europe-west4", "australia-southeast1"]


SYNTH = ["ra", "rb", "rc", "rd", "rq"]  # the synthetic planet's regions (name order = index order)
_PLANETS = {}


def synth_planet(tmp_path_factory):
    """(Planet, directory) of the synthetic planet: pings of 2 ms (1 ms one
    way), 1000 ms between the first and the last region."""
    if "synth" not in _PLANETS:
        d = str(tmp_path_factory.mktemp("planet"))
        for a in SYNTH:
            with open(os.path.join(d, a + ".dat"), "w") as f:
                for b in SYNTH:
                    ms = 0.1 if a == b else (1000.0 if {a, b} == {"ra", "rq"} else 2.0)
                    f.write("%.3f/%.3f/%.3f/0.100:%s\n" % (ms, ms, ms, b))
        _PLANETS["synth"] = (S.Planet(d), d)
    return _PLANETS["synth"]


def _planet(regions, tmp_path_factory):
    """(Planet for the GPU, planet directory for the oracle or None: the default)"""
    return synth_planet(tmp_path_factory) if regions is SYNTH else (planet(), None)


def _spec(regions, cmds, inst, pl=None):
    regs = (pl or planet()).ids(regions)
    return S.spec(S.EPAXOS, 5, 2, regs, regs, commands_per_client=cmds, conflict_rate=100, seed=32, instance=inst)


def site_lines(func):
    """Line numbers of the `fail_cap(__LINE__)` sites inside Sim::`func`."""
    src = os.path.join(os.path.dirname(os.path.abspath(S.__file__)), "csrc", "sim_wave.hip")
    lines = open(src).read().splitlines()
    start = [i for i, l in enumerate(lines) if "__device__" in l and re.search(r"\b%s\(" % func, l)]
    assert len(start) == 1, (func, start)
    out = set()
    for i in range(start[0] + 1, len(lines)):
        if "__device__ __forceinline__" in lines[i]:
            break
        if "fail_cap(__LINE__)" in lines[i]:
            out.add(i + 1)
    assert out
    return out


def site(res, i):
    return int(res.stats[i, _lib.FX_SIM_STAT_ERR_SITE])


_ORACLE = {}


def oracle(regions, cmds, inst, pl=None, pdir=None):
    """The oracle's output of one instance, computed once and shared (read only)."""
    key = (tuple(regions), cmds, inst)
    if key not in _ORACLE:
        s = _spec(regions, cmds, inst, pl)
        (o,) = O.sim_batch([to_oracle(s)], threads=1, **({"planet_dir": pdir} if pdir else {}))
        assert o["status"] == 0
        _ORACLE[key] = o
    return _ORACLE[key]


_THRESHOLD = {}


def smallest_passing(kind, lo, hi):
    """The smallest table size in (lo, hi] with which the GCP5 instance runs
    through on one fx_sim_run, by bisection (lo fails, hi passes: a larger
    table never fails where a smaller one passes); the size below it fails."""
    if kind not in _THRESHOLD:
        f = _spec(S.GCP5, 30, 0)
        err = lambda v: int(S.run([f], planet(), tiered=False, **{kind: v}).err[0])
        assert err(lo) == _lib.FX_ERR_SIM_CAPACITY and err(hi) == 0
        while hi - lo > 1:
            mid = (lo + hi) // 2
            e = err(mid)
            assert e in (0, _lib.FX_ERR_SIM_CAPACITY)
            lo, hi = (lo, mid) if e == 0 else (mid, hi)
        print(kind, "smallest passing", hi)
        assert err(hi) == 0 and err(hi - 1) == _lib.FX_ERR_SIM_CAPACITY
        _THRESHOLD[kind] = hi
    return _THRESHOLD[kind]


def failure(case):
    """(regions, commands per client, run arguments, expected status, builds
    (generic flags), the function whose fail_cap site is expected)"""
    if case == "pool_fixed":
        return FAR, 30, {}, _lib.FX_ERR_SIM_CAPACITY, (False, True), "send_batch_"
    if case == "pool_ring":
        return S.GCP5, 30, {"ring_entries": smallest_passing("ring_entries", 4, 80) - 1}, \
            _lib.FX_ERR_SIM_CAPACITY, (True,), "send_batch_"
    if case == "dots":
        return S.GCP5, 30, {"dot_slots": smallest_passing("dot_slots", 2, 64) - 1}, \
            _lib.FX_ERR_SIM_CAPACITY, (True,), "h_submit"
    if case == "xslots":
        return SYNTH, 6, {}, _lib.FX_ERR_SIM_CAPACITY, (False,), "insert_vertex"
    assert case == "events"
    return S.GCP5, 30, {"max_events": 500}, _lib.FX_ERR_SIM_EVENTS, (False, True), None


CASES = ["pool_fixed", "pool_ring", "dots", "xslots", "events"]


def rows(res, i):
    return (res.executed_len[i], res._executed[i], res._dot_client[i], res._lat[i], res.stats[i], res.err[i])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_failed_instance_ends_the_same_everywhere(case, tmp_path_factory):
    regions, cmds, kw, status, builds, func = failure(case)
    pl, pdir = _planet(regions, tmp_path_factory)
    f = _spec(regions, cmds, 2, pl)
    ok = [_spec(regions, 1, i, pl) for i in (0, 1, 3, 4)]
    ok_orc = [oracle(regions, 1, i, pl, pdir) for i in (0, 1, 3, 4)]
    per_build = []
    for generic in builds:
        alone = S.run([f], pl, tiered=False, generic=generic, **kw)
        print(case, "generic" if generic else "compiled-in", "status", int(alone.err[0]), "site", site(alone, 0),
              "executed", int(alone.executed_len[0].sum()), "events", alone.events(0))
        assert int(alone.err[0]) == status
        if status == _lib.FX_ERR_SIM_CAPACITY:
            assert site(alone, 0) in site_lines(func)
        else:
            assert alone.events(0) == 500 and site(alone, 0) == 0
        again = S.run([f], pl, tiered=False, generic=generic, **kw)
        same_buffers(alone, again)
        # in the middle of passing instances, and those without it
        mid = S.run(ok[:2] + [f] + ok[2:], pl, tiered=False, generic=generic, **kw)
        cap = alone.exec_cap
        okrun = S.run(ok, pl, tiered=False, generic=generic, exec_cap=cap, lat_cap=cmds, **kw)
        assert [int(e) for e in mid.err] == [0, 0, status, 0, 0] and not okrun.err.any()
        assert mid.exec_cap == cap
        for a, b in zip(rows(mid, 2), rows(alone, 0)):
            assert np.array_equal(a, b)
        for j, i in enumerate((0, 1, 3, 4)):
            assert_instance_parity(mid, i, ok[j], ok_orc[j])
            for a, b in zip(rows(mid, i), rows(okrun, j)):  # whole rows: the tails past the logs' ends too
                assert np.array_equal(a, b)
        # the neighbours' own samples plus the failed instance's partial ones
        assert np.array_equal(mid.delay, okrun.delay + alone.delay)
        assert np.array_equal(mid.chain, okrun.chain + alone.chain)
        assert np.array_equal(mid.latency_hist, okrun.latency_hist + alone.latency_hist)
        per_build.append(alone)
    if len(per_build) == 2:  # the two builds fail at the same place with the same rows
        same_buffers(per_build[0], per_build[1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES[:4])
def test_tiered_rerun_ends_equal_to_the_oracle(case, tmp_path_factory):
    regions, cmds, kw, status, builds, func = failure(case)
    pl, pdir = _planet(regions, tmp_path_factory)
    specs = [_spec(regions, 1, 0, pl), _spec(regions, cmds, 2, pl), _spec(regions, 1, 4, pl)]
    orc = [oracle(regions, 1, 0, pl, pdir), oracle(regions, cmds, 2, pl, pdir), oracle(regions, 1, 4, pl, pdir)]
    for generic in builds:
        res = S.run(specs, pl, generic=generic, **kw)
        assert not res.err.any() and res.reruns >= 1
        for i, (s, o) in enumerate(zip(specs, orc)):
            assert_instance_parity(res, i, s, o)
        hists_vs_oracle(res, orc)
