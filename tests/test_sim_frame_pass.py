"""One handler-loop pass per frame in the all-on-chip simulator (k_sim):
Sim::run_handlers_ pushes a frame, runs its handler and the executor on what
it committed, and visits the frame in the same iteration (its sends, a
self-delivery handed on, or its ready results and the pop).  The compiled-in
builds carry the frame's word and dot as values of that pass and touch the
frame lanes only around a nested frame.

Every case is computed once on the simulator oracle and compared with it on
the compiled-in build where the geometry has one and on the run-time build
(generic=True): orders, fast / slow / stable, events, trace, end time, latency
sums and the three histograms; the two builds buffer by buffer.  GCP regions,
one client per region and one key per command unless said, 20 commands per
client or fewer:

  atlas_n3     Atlas n = 3 f = 1, {2, 100} %: Submit -> own MCollect -> own
               MCollectAck (three frames deep), the commit to all from the
               deciding ack
  epaxos_n5    EPaxos n = 5 f = 2, {0, 50, 100} %: the headline build; leaf
               frames (remote MCollect / MCommit), the deciding ack's frame
               whose nested own MCommit executes and schedules the client's
               result before the parent's remaining targets are sent
  atlas_n7     Atlas n = 7 f = 2, {10, 100} %: next-target fields past 4,
               targets of 7 bits
  slow_path    EPaxos n = 5 f = 2 at 100 %, seed 44 (the oracle: 66 of the 100
               commands take the slow path): frames that carry MConsensus and
               MConsensusAck (the run's own stats must say slow > 0)
  two_results  2 clients per region, 2 keys per command from a pool of 2,
               100 %, the run-time build: both clients of a region wait at
               one process, a commit there executes a chain that holds a
               command of each, and the frame schedules two ready results
               (194 such frames; a build that drops a frame's second result
               fails here, profiles/sim_frame_pass.md)
  nested       one EPaxos n = 5 instance alone and at each place of a launch
               of three: the same rows everywhere
  ties         EPaxos n = 5 f = 2, {0, 100} %, 10 commands, on a synthetic
               planet (written under tmp_path): five process regions 50 ms
               apart, each client in a region of its own 50 ms from its
               process.  A result scheduled by a nested frame and the parent's
               remaining sends then arrive in the same millisecond, so their
               insertion order (the nested frame first) decides the order of
               the events, which the trace hash and the orders record
"""
import os

import numpy as np
import pytest

from fantoch_amd import sim as S
from oracle import oracle_lib as O
from test_sim_gpu import assert_instance_parity, planet, to_oracle
from test_sim_percmd_paths import hists_vs_oracle, same_buffers

CMDS = 20


def _atlas_n3():
    regs = planet().ids(S.GCP5[:3])
    return [S.spec(S.ATLAS, 3, 1, regs, regs, commands_per_client=CMDS, conflict_rate=c, seed=41, instance=i)
            for i, c in enumerate([2, 100])]


def _epaxos_n5():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, commands_per_client=CMDS, conflict_rate=c, seed=42, instance=i)
            for i, c in enumerate([0, 50, 100])]


def _atlas_n7():
    regs = list(range(0, 14, 2))  # 7 of the planet's regions
    return [S.spec(S.ATLAS, 7, 2, regs, regs, commands_per_client=CMDS, conflict_rate=c, seed=43, instance=i)
            for i, c in enumerate([10, 100])]


def _slow_path():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, commands_per_client=CMDS, conflict_rate=100, seed=44, instance=0)]


def _two_results():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, clients_per_region=2, commands_per_client=CMDS, conflict_rate=100,
                   keys_per_command=2, pool_size=2, seed=45, instance=i) for i in range(2)]


def _nested():
    """The instance under test first, then its two neighbours (the same shape:
    the launches' log capacities do not depend on who is in them)."""
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, commands_per_client=10, conflict_rate=c, seed=46, instance=i)
            for i, c in enumerate([50, 0, 100])]


CASES = {"atlas_n3": _atlas_n3, "epaxos_n5": _epaxos_n5, "atlas_n7": _atlas_n7, "slow_path": _slow_path,
         "two_results": _two_results, "nested": _nested}
_ORACLE = {}


def oracle(case):
    """(specs, oracle outputs) of a case, computed once and shared (read only)."""
    if case not in _ORACLE:
        specs = CASES[case]()
        orc = O.sim_batch([to_oracle(s) for s in specs], threads=8)
        assert all(o["status"] == 0 for o in orc)
        _ORACLE[case] = (specs, orc)
    return _ORACLE[case]


def vs_oracle(res, specs, orc):
    assert not res.err.any(), [int(e) for e in res.err]
    assert res.reruns == 0
    for i, (s, o) in enumerate(zip(specs, orc)):
        assert_instance_parity(res, i, s, o)
    hists_vs_oracle(res, orc)


def on_both_builds(specs, orc):
    fixed = S.run(specs, planet())
    vs_oracle(fixed, specs, orc)
    generic = S.run(specs, planet(), generic=True)
    vs_oracle(generic, specs, orc)
    same_buffers(fixed, generic)
    return fixed, generic


def test_oracle_exercises_the_paths():
    """The cases' claims as far as the oracle's output shows them."""
    specs, orc = oracle("epaxos_n5")
    by_rate = {s.conflict_rate: o for s, o in zip(specs, orc)}
    assert by_rate[0]["slow"].sum() == 0 and by_rate[0]["fast"].sum() == 5 * CMDS
    assert by_rate[0]["chain"][1] > 0  # Adds that execute in the frame of the commit
    assert by_rate[100]["chain"][2:].sum() > 0  # and chains released later
    specs, orc = oracle("slow_path")
    print("slow_path: fast %s slow %s" % (list(orc[0]["fast"]), list(orc[0]["slow"])))
    assert orc[0]["slow"].sum() > 0
    specs, orc = oracle("two_results")
    for s, o in zip(specs, orc):
        print("two_results: chains %s" % list(o["chain"][:12]))
        assert o["chain"][2:].sum() > 0  # chains of several commands executed by one Add
    specs, orc = oracle("nested")
    assert orc[0]["fast"].sum() > 0 and orc[0]["chain"][1] > 0
    specs, orc = oracle("atlas_n7")
    assert all(int(f) + int(w) > 0 for o in orc for f, w in zip(o["fast"], o["slow"]))  # every process coordinates


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["atlas_n3", "epaxos_n5", "atlas_n7"])
def test_paths_match_the_oracle_on_both_builds(case):
    on_both_builds(*oracle(case))


@pytest.mark.gpu
def test_slow_path_frames():
    specs, orc = oracle("slow_path")
    for res in on_both_builds(specs, orc):
        slow = int(sum(res.slow(0)))
        print("slow paths", slow)
        assert slow > 0


@pytest.mark.gpu
def test_several_ready_results_in_one_frame():
    specs, orc = oracle("two_results")
    res = S.run(specs, planet())  # 10 clients: the run-time build whatever is asked
    vs_oracle(res, specs, orc)
    generic = S.run(specs, planet(), generic=True)
    vs_oracle(generic, specs, orc)
    same_buffers(res, generic)


TIE_P = ["pa", "pb", "pc", "pd", "pe"]
TIE_C = ["ca", "cb", "cc", "cd", "ce"]
_TIES = {}


def tie_planet(tmp_path_factory):
    """(Planet, directory): pings of 100 ms (50 ms one way) between the process
    regions and between client region k and process region k, 300 ms elsewhere."""
    if "planet" not in _TIES:
        d = str(tmp_path_factory.mktemp("tie_planet"))
        for a in TIE_P + TIE_C:
            with open(os.path.join(d, a + ".dat"), "w") as f:
                for b in TIE_P + TIE_C:
                    near = (a in TIE_P and b in TIE_P) or (a[0] != b[0] and a[1] == b[1])
                    ms = 0.1 if a == b else (100.0 if near else 300.0)
                    f.write("%.3f/%.3f/%.3f/0.100:%s\n" % (ms, ms, ms, b))
        _TIES["planet"] = (S.Planet(d), d)
    return _TIES["planet"]


@pytest.mark.gpu
def test_insertion_order_decides_events_of_one_millisecond(tmp_path_factory):
    pl, d = tie_planet(tmp_path_factory)
    specs = [S.spec(S.EPAXOS, 5, 2, pl.ids(TIE_P), pl.ids(TIE_C), commands_per_client=10, conflict_rate=c, seed=47,
                    instance=i) for i, c in enumerate([0, 100])]
    orc = O.sim_batch([to_oracle(s) for s in specs], threads=2, planet_dir=d)
    assert all(o["status"] == 0 for o in orc)
    fixed = S.run(specs, pl)
    vs_oracle(fixed, specs, orc)
    generic = S.run(specs, pl, generic=True)
    vs_oracle(generic, specs, orc)
    same_buffers(fixed, generic)


def rows(res, i):
    return (res.executed_len[i], res._executed[i], res._dot_client[i], res._lat[i], res.stats[i], res.err[i])


@pytest.mark.gpu
@pytest.mark.parametrize("generic", [False, True])
def test_nested_frames_end_the_same_alone_and_between_instances(generic):
    """The Submit's frames (own MCollect, own MCollectAck) and the deciding
    ack's (own MCommit whose Add executes) of one instance: equal to the oracle
    alone, and word for word the same rows first, in the middle and last in a
    launch of three."""
    specs, orc = oracle("nested")
    x, a, b = specs
    alone = S.run([x], planet(), generic=generic)
    vs_oracle(alone, [x], orc[:1])
    for order in ([0, 1, 2], [1, 0, 2], [1, 2, 0]):
        res = S.run([specs[j] for j in order], planet(), generic=generic)
        vs_oracle(res, [specs[j] for j in order], [orc[j] for j in order])
        assert res.exec_cap == alone.exec_cap
        for u, v in zip(rows(res, order.index(0)), rows(alone, 0)):
            assert np.array_equal(u, v)
