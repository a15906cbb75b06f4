"""The GC ring of the all-on-chip simulator (k_sim): every pair (process,
source) keeps ONE time-keyed ring of its committed frontier's last moves
(h_mcommitdot), and gc_finish evaluates the Stable counts from the rings: a
process's own frontier at its last GC delivery and the frontier a tick
reported are the same look-up, the newest entry at or before a time.  The
tick index no longer exists in the kernel: a tick's report is the look-up at
the tick's own time, so GC intervals that divide nothing evenly need no
division on the commit path and are checked here through the counts alone.

Every case runs on the compiled-in build where the geometry has one and on the
run-time build (generic=True): Stable counters, trace, event count and end time
equal the simulator oracle's, and the two builds agree buffer by buffer.

  epaxos / atlas, n = 3 / 5   20 commands per client at 50 % conflicts, a tick
               every 1, 7, 10 and 1000 ms, without extra simulated time and
               with 50 ms of it (the run then ends on a GC action).  20 commits
               per source go round a six-entry ring several times
  atlas_n7     Atlas n = 7 f = 2, 10 commands per client (its own compiled-in
               build)
  gc off       gc_interval_ms = 0: nothing is logged and no instance fails
  lost entry   a synthetic planet (written under tmp_path): processes pa, pb,
               pc 20 ms apart and pf 250 ms from all of them, clients 1 ms
               from pa, pb, pc.  A source commits every 44 ms, so the 250 ms a
               report travels to or from pf hold more moves than the ring's
               six entries: tests/gc_ring_ref.py, fed with the oracle's commit
               times, says which instances lose an entry (those with pf) and
               which do not.  Exactly those fail the first launch with
               FX_ERR_SIM_CAPACITY, are rerun on the larger tables' deeper ring
               by fx_sim_run_tiered and equal the oracle
  poison       one of the batches above with the register file filled with
               tagged garbage and with zeros before the launch
               (tests/test_sim_poison.py's fills)
"""
import os

import numpy as np
import pytest

import gc_ring_ref as R
from fantoch_amd import _lib
from fantoch_amd import sim as S
from oracle import oracle_lib as O
from test_sim_gpu import assert_instance_parity, planet, to_oracle
from test_sim_percmd_paths import hists_vs_oracle, same_buffers
from test_sim_poison import FILLS, poisoner

GC_MS = [1, 7, 10, 1000]
CASES = {"epaxos_n5": (S.EPAXOS, 5, 2, 20), "epaxos_n3": (S.EPAXOS, 3, 1, 20), "atlas_n5": (S.ATLAS, 5, 2, 20),
         "atlas_n3": (S.ATLAS, 3, 1, 20), "atlas_n7": (S.ATLAS, 7, 2, 10)}
_ORACLE = {}


def batch(case):
    """(specs, oracle outputs), computed once and shared (read only): every
    interval without and with 50 ms of extra simulated time."""
    if case not in _ORACLE:
        proto, n, f, cmds = CASES[case]
        regs = list(range(0, 14, 2)) if n == 7 else planet().ids(S.GCP5[:n])
        specs = [S.spec(proto, n, f, regs, regs, commands_per_client=cmds, conflict_rate=50, gc_interval_ms=gc,
                        extra_sim_time_ms=extra, seed=53, instance=i)
                 for i, (gc, extra) in enumerate((gc, extra) for extra in (-1, 50) for gc in GC_MS)]
        orc = O.sim_batch([to_oracle(s) for s in specs], threads=8)
        assert all(o["status"] == 0 for o in orc)
        _ORACLE[case] = (specs, orc)
    return _ORACLE[case]


def vs_oracle(res, specs, orc):
    """Every instance and the batch histograms against the oracle.  An
    instance whose ring lost an entry is rerun with larger tables
    (fx_sim_run_tiered), so reruns are allowed and errors are not."""
    bad = [(i, int(e), int(res.stats[i, _lib.FX_SIM_STAT_ERR_SITE])) for i, e in enumerate(res.err) if e]
    assert not bad, "instances failed (instance, error, site): %s" % bad[:8]
    print("reruns", res.reruns)
    for i, (s, o) in enumerate(zip(specs, orc)):
        assert_instance_parity(res, i, s, o)
    hists_vs_oracle(res, orc)


def on_both_builds(specs, orc, pl=None):
    pl = pl or planet()
    fixed = S.run(specs, pl)
    vs_oracle(fixed, specs, orc)
    generic = S.run(specs, pl, generic=True)
    vs_oracle(generic, specs, orc)
    same_buffers(fixed, generic)
    return fixed, generic


def test_oracle_stabilises_under_every_interval():
    """The cases mean something: every run stabilises commands, and the
    counts differ between the intervals."""
    for case in CASES:
        specs, orc = batch(case)
        stable = {(s.gc_interval_ms, s.extra_sim_time_ms): int(sum(o["stable"])) for s, o in zip(specs, orc)}
        print(case, stable)
        assert min(stable.values()) > 0
        assert len(set(stable.values())) > 2


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_stable_counts_match_the_oracle_on_both_builds(case):
    on_both_builds(*batch(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["epaxos_n5", "atlas_n3"])
def test_gc_off_logs_nothing_and_never_fails(case):
    proto, n, f, cmds = CASES[case]
    regs = planet().ids(S.GCP5[:n])
    specs = [S.spec(proto, n, f, regs, regs, commands_per_client=cmds, conflict_rate=c, gc_interval_ms=0, seed=54,
                    instance=i) for i, c in enumerate([0, 50, 100])]
    orc = O.sim_batch([to_oracle(s) for s in specs], threads=4)
    assert all(o["status"] == 0 and int(sum(o["stable"])) == 0 for o in orc)
    for res in on_both_builds(specs, orc):
        assert res.reruns == 0 and not res.err.any()


# ------------------------------------------------------------ a lost entry
FAR_P = ["pa", "pb", "pc", "pf"]
FAR_C = ["ca", "cb", "cc"]
_FAR = {}


def far_planet(tmp_path_factory):
    """(Planet, directory): pings of 40 ms between pa, pb, pc and the clients'
    regions, 2 ms between client region k and process region k, 500 ms to pf."""
    if "planet" not in _FAR:
        d = str(tmp_path_factory.mktemp("far_planet"))
        for a in FAR_P + FAR_C:
            with open(os.path.join(d, a + ".dat"), "w") as f:
                for b in FAR_P + FAR_C:
                    if a == b:
                        ms = 0.1
                    elif "pf" in (a, b):
                        ms = 500.0
                    else:
                        ms = 2.0 if (a[0] != b[0] and a[1] == b[1]) else 40.0
                    f.write("%.3f/%.3f/%.3f/0.100:%s\n" % (ms, ms, ms, b))
        _FAR["planet"] = (S.Planet(d), d)
    return _FAR["planet"]


def far_batch(tmp_path_factory):
    """(specs, oracle outputs, which instances the reference says lose an
    entry): EPaxos n = 3, two clients; the instances on (pa, pb, pf) and on
    (pa, pb, pc) alternate, under a 10 ms and a 50 ms interval."""
    if "batch" not in _FAR:
        pl, d = far_planet(tmp_path_factory)
        specs = [S.spec(S.EPAXOS, 3, 1, pl.ids(["pa", "pb", third]), pl.ids(["ca", "cb"]), commands_per_client=20,
                        conflict_rate=50, gc_interval_ms=gc, seed=51, instance=i)
                 for i, (gc, third) in enumerate((gc, third) for gc in (10, 50) for third in ("pf", "pc", "pf", "pc"))]
        orc = O.sim_batch([to_oracle(s) for s in specs], threads=4, planet_dir=d)
        assert all(o["status"] == 0 for o in orc)
        lost = []
        for s, o in zip(specs, orc):
            n = s.n
            streams, _ = O.sim_capture(to_oracle(s), planet_dir=d)
            hist = R.histories_from_adds(n, streams)
            delay = [[int(pl.ping[s.process_regions[p], s.process_regions[q]]) // 2 for q in range(n)] for p in range(n)]
            depth = R.ring_depth(n, s.clients_per_region * s.num_client_regions)
            rings = [[R.ring_of(h, depth) for h in row] for row in hist]
            ok, got = R.finish_ring(n, rings, delay, s.gc_interval_ms, o["end_ms"])
            gone, want = R.finish_brute(n, hist, delay, s.gc_interval_ms, o["end_ms"], depth=depth)
            # the reference's evaluation of the oracle's commit times is the oracle's own count
            assert want == [int(x) for x in o["stable"][:n]]
            assert ok == (not gone) and (not ok or got == want)
            # the rerun geometry's ring holds what the first launch's lost
            deep = R.ring_depth(n, s.clients_per_region * s.num_client_regions, wslots=256)
            assert R.finish_ring(n, [[R.ring_of(h, deep) for h in row] for row in hist], delay, s.gc_interval_ms,
                                 o["end_ms"]) == (True, want)
            lost.append(not ok)
        _FAR["batch"] = (specs, orc, lost)
    return _FAR["batch"]


def test_reference_loses_the_entry_behind_the_far_replica(tmp_path_factory):
    """On the CPU: exactly the instances with pf lose an entry of a six-entry ring."""
    specs, orc, lost = far_batch(tmp_path_factory)
    pl, _ = far_planet(tmp_path_factory)
    far = [pl.index["pf"] in list(s.process_regions[:s.n]) for s in specs]
    print("lost", lost)
    assert lost == far and any(lost) and not all(lost)


@pytest.mark.gpu
def test_lost_entries_rerun_on_the_deeper_ring(tmp_path_factory):
    specs, orc, lost = far_batch(tmp_path_factory)
    pl, _ = far_planet(tmp_path_factory)
    for generic in (False, True):
        first = S.run(specs, pl, generic=generic, tiered=False)
        failed = [int(e) != 0 for e in first.err]
        print("first launch", [int(e) for e in first.err])
        assert failed == lost
        assert all(int(e) == _lib.FX_ERR_SIM_CAPACITY for e, x in zip(first.err, lost) if x)
    fixed, generic = on_both_builds(specs, orc, pl)
    assert fixed.reruns == sum(lost) and generic.reruns == sum(lost)


@pytest.mark.gpu
@pytest.mark.parametrize("generic", [False, True])
def test_poisoned_registers_do_not_change_the_counts(generic):
    specs, orc = batch("epaxos_n5")
    for mode, tag in FILLS:
        res = S.run(specs, planet(), generic=generic, before_launch=poisoner(mode, tag))
        vs_oracle(res, specs, orc)
