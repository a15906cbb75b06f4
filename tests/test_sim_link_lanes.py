"""The process links of the compiled-in simulator builds (k_sim, GeoCT::link_d):
link l's messages in flight live in registers of lane l, D = 4 entries of
(time, insertion seq, payload), instead of the LDS pool.  EPaxos n = 5 f = 2
and Atlas n = 3 f = 1 (one client per region) have their links in lanes; the
Atlas n = 5 and n = 7 builds of the placement sweep keep the pool (a far
replica puts up to 24 messages on a link there) and are run here all the same.
What a link's fifth message does is a trait of the build (GeoCT::link_ovf).
Atlas n = 3: it stops the instance with FX_ERR_SIM_CAPACITY and
fx_sim_run_tiered reruns it on the run-time build, which keeps the pool.
EPaxos n = 5: it goes to the link's overflow list in the pool, the capacity
stays the pool's (80 messages in flight), and the build stops exactly where the
run-time build stops (tests/test_sim_loop_exits.py's pool_fixed case holds it
to that).
tests/link_ring_ref.py restates the ring on the CPU
(tests/test_sim_link_lanes_ref.py).

  parity    every compiled-in geometry, one client per region on the GCP
            regions, 20-50 commands per client, conflict rates 0, 2, 10, 50 and
            100 %: orders, Fast / Slow / Stable, trace, event count, end time,
            latencies and the three batch histograms equal the simulator
            oracle's, and every buffer equals the run-time build's
            (FX_SIM_FLAG_GENERIC).  The geometries with links in lanes do it
            without a rerun
  fit       a synthetic planet (written under tmp_path): processes pa, pb and a
            third region NNN ms from everything, Atlas n = 3 f = 1, 100 %
            conflicts, GC off.  tools/sim_link_depth.py --far (the profile
            build's depth stat, stat 31, on the pool build) gives the deepest
            link of each: 3 at 80 ms, 4 = D at 120 ms, 5 = D + 1 at 130 ms.
            The first two pass the first launch; the third stops it with
            FX_ERR_SIM_CAPACITY on the compiled-in build only (the pool of the
            run-time build holds it), is rerun by fx_sim_run_tiered, counted in
            `reruns`, and equals the oracle.  A fourth, 130 ms with 8 commands
            per client (the same depth, 5), has no more dots than the dot table
            has slots: a send that dropped its message in silence would not run
            into another table later, it would end the first launch without an
            error
  overflow  EPaxos n = 5 on the europe-west regions with Sydney as the far
            replica, 4 to 30 commands per client: links run deeper than D (the
            profile build's depth stat on these specs: 8 to 17), the
            lanes spill to their lists in the pool and refill from them.  One
            fx_sim_run gives the same buffers as the run-time build, the
            instances that fill the pool included (the same event, the same
            site); those that pass equal the oracle; through fx_sim_run_tiered
            all do
  poison    the EPaxos batch, and the overflow batch, with the register file
            filled with 0xA5-tagged garbage and with zeros before the launch
            (tests/test_sim_poison.py's helper): the link registers are written
            before they are read
"""
import os

import pytest

from fantoch_amd import _lib
from fantoch_amd import sim as S
from oracle import oracle_lib as O
from test_sim_gpu import assert_instance_parity, planet, to_oracle
from test_sim_percmd_paths import hists_vs_oracle, same_buffers
from test_sim_poison import poisoner

pytestmark = pytest.mark.gpu

RATES = [0, 2, 10, 50, 100]
# protocol, n, f, commands per client, links in lanes
CASES = {"epaxos_n5_f2": (S.EPAXOS, 5, 2, 50, True), "atlas_n3_f1": (S.ATLAS, 3, 1, 50, True),
         "atlas_n5_f1": (S.ATLAS, 5, 1, 30, False), "atlas_n5_f2": (S.ATLAS, 5, 2, 30, False),
         "atlas_n7_f1": (S.ATLAS, 7, 1, 20, False), "atlas_n7_f2": (S.ATLAS, 7, 2, 20, False)}
_ORACLE = {}


def batch(case):
    """(specs, oracle outputs), computed once and shared (read only)."""
    if case not in _ORACLE:
        proto, n, f, cmds, _ = CASES[case]
        regs = list(range(0, 14, 2)) if n == 7 else planet().ids(S.GCP5[:n])
        specs = [S.spec(proto, n, f, regs, regs, commands_per_client=cmds, conflict_rate=c, seed=20250213, instance=i)
                 for i, c in enumerate(RATES)]
        orc = O.sim_batch([to_oracle(s) for s in specs], threads=8)
        assert all(o["status"] == 0 for o in orc)
        _ORACLE[case] = (specs, orc)
    return _ORACLE[case]


def vs_oracle(res, specs, orc):
    bad = [(i, int(e), int(res.stats[i, _lib.FX_SIM_STAT_ERR_SITE])) for i, e in enumerate(res.err) if e]
    assert not bad, "instances failed (instance, error, site): %s" % bad[:8]
    for i, (s, o) in enumerate(zip(specs, orc)):
        assert_instance_parity(res, i, s, o)
    hists_vs_oracle(res, orc)


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_the_oracle_and_the_run_time_build(case):
    specs, orc = batch(case)
    fixed = S.run(specs, planet())
    vs_oracle(fixed, specs, orc)
    print("reruns", fixed.reruns)
    if CASES[case][4]:
        assert fixed.reruns == 0
    generic = S.run(specs, planet(), generic=True)
    vs_oracle(generic, specs, orc)
    same_buffers(fixed, generic)


# ------------------------------------------------------- fit / exceed at D
# (far region's distance in ms, commands per client): the deepest link holds
# 3, 4 = D, 5 = D + 1 and 5 messages
FAR = [(80, 20), (120, 20), (130, 20), (130, 8)]
FAR_MS = sorted({ms for ms, _ in FAR})
_FAR = {}


def far_batch(tmp_path_factory):
    """(Planet, specs, oracle outputs): the planet of tools/sim_link_depth.py
    --far with the pinned distances."""
    if not _FAR:
        d = str(tmp_path_factory.mktemp("far_links"))
        names = ["pa", "pb", "ca", "cb", "cc"] + ["f%03d" % ms for ms in FAR_MS]
        for x in names:
            with open(os.path.join(d, x + ".dat"), "w") as f:
                for y in names:
                    if x == y:
                        ms = 0.1
                    elif x[0] == "f" or y[0] == "f":
                        ms = float(max(int(z[1:]) for z in (x, y) if z[0] == "f"))
                    else:
                        ms = 2.0 if (x[0] != y[0] and x[1] == y[1]) else 40.0
                    f.write("%.3f/%.3f/%.3f/0.100:%s\n" % (ms, ms, ms, y))
        pl = S.Planet(d)
        specs = [S.spec(S.ATLAS, 3, 1, pl.ids(["pa", "pb", "f%03d" % ms]), pl.ids(["ca", "cb", "cc"]),
                        commands_per_client=cmds, conflict_rate=100, gc_interval_ms=0, seed=61, instance=i)
                 for i, (ms, cmds) in enumerate(FAR)]
        orc = O.sim_batch([to_oracle(s) for s in specs], threads=4, planet_dir=d)
        assert all(o["status"] == 0 for o in orc)
        _FAR["batch"] = (pl, specs, orc)
    return _FAR["batch"]


def test_a_link_of_depth_d_fits_and_d_plus_one_is_rerun(tmp_path_factory):
    pl, specs, orc = far_batch(tmp_path_factory)
    cap = _lib.FX_ERR_SIM_CAPACITY
    first = S.run(specs, pl, tiered=False)
    print("first launch", [int(e) for e in first.err], [int(x) for x in first.stats[:, _lib.FX_SIM_STAT_ERR_SITE]])
    assert [int(e) for e in first.err] == [0, 0, cap, cap]
    for i in (0, 1):
        assert_instance_parity(first, i, specs[i], orc[i])
    # the run-time build keeps the pool: nothing stops its first launch
    pool = S.run(specs, pl, tiered=False, generic=True)
    assert not pool.err.any()
    vs_oracle(pool, specs, orc)
    # capacity is never terminal
    tiered = S.run(specs, pl)
    vs_oracle(tiered, specs, orc)
    assert tiered.reruns == 2
    generic = S.run(specs, pl, generic=True)
    assert generic.reruns == 0
    vs_oracle(generic, specs, orc)


@pytest.mark.parametrize("fill", [(1, 0xA5), (4, 0)], ids=["a5", "zero"])
def test_link_registers_are_written_before_they_are_read(fill):
    specs, orc = batch("epaxos_n5_f2")
    res = S.run(specs, planet(), before_launch=poisoner(*fill))
    vs_oracle(res, specs, orc)
    assert res.reruns == 0


# ------------------------------------------ the overflow list (EPaxos n = 5)
# the europe-west regions with one far replica (Sydney): the links to and from
# it hold more than D messages (tools/sim_link_depth.py's stat on these specs:
# see the docstring), so the lanes spill to their lists in the pool and refill
SYDNEY = ["europe-west1", "europe-west2", "europe-west3", "europe-west4", "australia-southeast1"]
_SYDNEY = {}


def sydney_batch():
    if not _SYDNEY:
        regs = planet().ids(SYDNEY)
        specs = [S.spec(S.EPAXOS, 5, 2, regs, regs, commands_per_client=cmds, conflict_rate=rate, seed=62, instance=i)
                 for i, (cmds, rate) in enumerate([(4, 100), (8, 100), (8, 0), (8, 50), (12, 100), (30, 100)])]
        orc = O.sim_batch([to_oracle(s) for s in specs], threads=8)
        assert all(o["status"] == 0 for o in orc)
        _SYDNEY["batch"] = (specs, orc)
    return _SYDNEY["batch"]


def test_full_link_lanes_spill_to_the_pool_and_stop_where_the_pool_is_full():
    specs, orc = sydney_batch()
    first = S.run(specs, planet(), tiered=False)
    pool = S.run(specs, planet(), tiered=False, generic=True)
    print("first launch", [int(e) for e in first.err], "events", [first.events(i) for i in range(len(specs))])
    # the same instances stop, at the same event, with the same rows: the
    # capacity is the pool's on both builds
    same_buffers(first, pool)
    assert set(int(e) for e in first.err) == {0, _lib.FX_ERR_SIM_CAPACITY}
    for i, (s, o) in enumerate(zip(specs, orc)):
        if not first.err[i]:
            assert_instance_parity(first, i, s, o)
    fixed = S.run(specs, planet())
    vs_oracle(fixed, specs, orc)
    generic = S.run(specs, planet(), generic=True)
    vs_oracle(generic, specs, orc)
    same_buffers(fixed, generic)
    assert fixed.reruns == generic.reruns == int((first.err != 0).sum())


@pytest.mark.parametrize("fill", [(1, 0xA5), (4, 0)], ids=["a5", "zero"])
def test_the_overflow_list_from_poisoned_registers(fill):
    specs, orc = sydney_batch()
    res = S.run(specs, planet(), before_launch=poisoner(*fill))
    vs_oracle(res, specs, orc)
