"""The event paths of the all-on-chip simulator (k_sim) that share one handler
call site: every process link, submit, executed-notification and client-reply
event funnels into the same run_handlers, and the lane selects of its helpers
are plain v_cndmask selects on a lane id read once per helper.  Each case runs
once on the compiled-in geometry build and once on the run-time geometry build
(generic=True); both must equal the simulator oracle bit for bit, exactly as
test_sim_gpu.run_and_compare checks it (orders, fast / slow / stable, events,
trace, end time, the three histograms), and each other.

GCP regions, one client per region, 30 commands per client: on the oracle
that is enough for both the fast path and MConsensus to run in the 50 % /
100 % instances of either protocol, and for the run with extra time to end
after the last client reply (test_oracle_exercises_the_paths checks it on the
oracle's output, not on the GPU's), so the count was not raised.

  epaxos_n5   configs[1] shape, conflicts {0, 50, 100} %, 4 instances each:
              every process coordinates (one client per region), so a
              coordinator's self-delivery is the first (id 1), a middle (3) and
              the last (5) of a frame's targets, and ready results are
              scheduled between a frame's sends
  atlas_n3    configs[0] shape at 2 % and 100 %: self MCollect -> self
              MCollectAck nesting (frame depth 3)
  atlas_n5    configs[2] shape: f = 1 and f = 2 in one batch (f per instance)
  atlas_n7    configs[2] shape, n = 7 f = 2 over 7 of the 20 regions: link
              lanes 42-48, 9 executor slots per process
  epaxos_extra  100 % conflicts and 50 ms of extra simulated time: the
              executed-notification links are simulated and end the run
"""
import numpy as np
import pytest

from fantoch_amd import sim as S
from oracle import oracle_lib as O
from test_sim_gpu import assert_instance_parity, planet, to_oracle

CMDS = 30


def _epaxos_n5():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, commands_per_client=CMDS, conflict_rate=c, seed=11, instance=i)
            for i, c in enumerate([0, 50, 100] * 4)]


def _atlas_n3():
    regs = planet().ids(S.GCP5[:3])
    return [S.spec(S.ATLAS, 3, 1, regs, regs, commands_per_client=CMDS, conflict_rate=c, seed=12, instance=i)
            for i, c in enumerate([2, 100, 2, 100])]


def _atlas_n5():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.ATLAS, 5, f, regs, regs, commands_per_client=CMDS, conflict_rate=c, seed=13, instance=i)
            for i, (f, c) in enumerate([(1, 50), (2, 50), (1, 100), (2, 100)])]


def _atlas_n7():
    sub = list(range(0, 20, 3))  # 7 of the planet's 20 regions
    assert len(sub) == 7 and planet().R == 20
    return [S.spec(S.ATLAS, 7, 2, sub, sub, commands_per_client=CMDS, conflict_rate=c, seed=14, instance=i)
            for i, c in enumerate([50, 100])]


def _epaxos_extra(extra=50):
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, commands_per_client=CMDS, conflict_rate=100,
                   extra_sim_time_ms=extra, seed=15, instance=i) for i in range(2)]


CASES = {"epaxos_n5": _epaxos_n5, "atlas_n3": _atlas_n3, "atlas_n5": _atlas_n5, "atlas_n7": _atlas_n7,
         "epaxos_extra": _epaxos_extra}
_ORACLE = {}


def oracle(case):
    """(specs, oracle outputs) of a case, computed once and shared."""
    if case not in _ORACLE:
        specs = CASES[case]()
        orc = O.sim_batch([to_oracle(s) for s in specs], threads=8)
        assert all(o["status"] == 0 for o in orc)
        _ORACLE[case] = (specs, orc)
    return _ORACLE[case]


def test_oracle_exercises_the_paths():
    """On the oracle's output: over the 50 % / 100 % instances of each
    protocol both the fast path and MConsensus ran, and the run with extra
    time ends after the last client reply (= where the same instance without
    extra time stops: a run without it ends on the last client's last reply)."""
    for cases in (("epaxos_n5", "epaxos_extra"), ("atlas_n3", "atlas_n5", "atlas_n7")):
        fast = slow = 0
        for case in cases:
            specs, orc = oracle(case)
            for s, o in zip(specs, orc):
                if s.conflict_rate in (50, 100):
                    fast += int(np.sum(o["fast"]))
                    slow += int(np.sum(o["slow"]))
        print(cases, "fast", fast, "slow", slow)
        assert fast > 0 and slow > 0
    specs, orc = oracle("epaxos_extra")
    plain = O.sim_batch([to_oracle(s) for s in _epaxos_extra(extra=-1)], threads=8)
    for o, o0 in zip(orc, plain):
        print("end_ms", o["end_ms"], "last client reply", o0["end_ms"])
        assert o0["status"] == 0 and o["end_ms"] > o0["end_ms"]


def vs_oracle(res, specs, orc):
    bad = [(i, int(e)) for i, e in enumerate(res.err) if e]
    assert not bad, "instances failed: %s" % bad[:8]
    for i, (s, o) in enumerate(zip(specs, orc)):
        assert_instance_parity(res, i, s, o)
    lat = sum(o["latency"] for o in orc)
    assert np.array_equal(res.latency_hist[:, :lat.shape[1]], lat[:, :res.latency_hist.shape[1]])
    assert np.array_equal(res.chain, sum(o["chain"] for o in orc)[:res.chain.shape[0]])
    assert np.array_equal(res.delay, sum(o["delay"] for o in orc)[:res.delay.shape[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_event_paths_match_the_oracle_on_both_builds(case):
    specs, orc = oracle(case)
    fixed = S.run(specs, planet())
    vs_oracle(fixed, specs, orc)
    generic = S.run(specs, planet(), generic=True)
    vs_oracle(generic, specs, orc)
    # the two builds against each other: every output buffer of the batch
    assert fixed.reruns == 0 and generic.reruns == 0
    assert np.array_equal(fixed.executed_len, generic.executed_len)
    for i in range(len(specs)):
        for a, b in zip(fixed.executed(i), generic.executed(i)):
            assert np.array_equal(a, b)
        assert np.array_equal(fixed.latencies(i), generic.latencies(i))
    assert np.array_equal(fixed.stats, generic.stats)
    assert np.array_equal(fixed.latency_hist, generic.latency_hist)
    assert np.array_equal(fixed.chain, generic.chain)
    assert np.array_equal(fixed.delay, generic.delay)
