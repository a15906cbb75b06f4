"""The GC tick index of the all-on-chip simulator (k_sim): h_mcommitdot logs,
for every move of a committed frontier, how many GC ticks lie strictly before
the current millisecond, (now - 1) / gc_interval_ms, and gc_finish evaluates
the Stable counts from those logs.  GC intervals that divide nothing evenly,
the BASELINE's 10 ms, a whole second (a handful of ticks in a run) and 1 ms (a
tick every millisecond), with and without extra simulated time (where the run
ends on a GC action), EPaxos and Atlas at n = 3 and n = 5, on the compiled-in
build where the geometry has one and on the run-time build: the Stable
counters, the trace, the event count and the end time equal the simulator
oracle's, and the two builds agree buffer by buffer.
"""
import pytest

from fantoch_amd import sim as S
from oracle import oracle_lib as O
from test_sim_gpu import assert_instance_parity, planet, to_oracle
from test_sim_percmd_paths import hists_vs_oracle, same_buffers

GC_MS = [1, 3, 7, 10, 1000]
CASES = {"epaxos_n5": (S.EPAXOS, 5, 2), "epaxos_n3": (S.EPAXOS, 3, 1), "atlas_n5": (S.ATLAS, 5, 2),
         "atlas_n3": (S.ATLAS, 3, 1)}
_ORACLE = {}


def batch(case):
    """(specs, oracle outputs), computed once and shared (read only): every
    interval without and with 50 ms of extra simulated time."""
    if case not in _ORACLE:
        proto, n, f = CASES[case]
        regs = planet().ids(S.GCP5[:n])
        specs = [S.spec(proto, n, f, regs, regs, commands_per_client=20, conflict_rate=50, gc_interval_ms=gc,
                        extra_sim_time_ms=extra, seed=41, instance=i)
                 for i, (gc, extra) in enumerate((gc, extra) for extra in (-1, 50) for gc in GC_MS)]
        orc = O.sim_batch([to_oracle(s) for s in specs], threads=8)
        assert all(o["status"] == 0 for o in orc)
        _ORACLE[case] = (specs, orc)
    return _ORACLE[case]


def test_oracle_sees_the_ticks():
    """The intervals matter to the oracle's own Stable counts: every run
    stabilises something, and the totals differ between the intervals."""
    for case in CASES:
        specs, orc = batch(case)
        stable = {(s.gc_interval_ms, s.extra_sim_time_ms): int(sum(o["stable"])) for s, o in zip(specs, orc)}
        print(case, stable)
        assert min(stable.values()) > 0
        assert len(set(stable.values())) > 2


def vs_oracle(res, specs, orc):
    """Every instance and the batch histograms against the oracle.  A tick
    every millisecond can outgrow the small tick log of the first launch
    (FX_ERR_SIM_CAPACITY); fx_sim_run_tiered reruns such an instance with
    larger tables, so reruns are allowed and errors are not."""
    bad = [(i, int(e)) for i, e in enumerate(res.err) if e]
    assert not bad, "instances failed: %s" % bad[:8]
    print("reruns", res.reruns)
    for i, (s, o) in enumerate(zip(specs, orc)):
        assert_instance_parity(res, i, s, o)
    hists_vs_oracle(res, orc)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_stable_counts_match_the_oracle_on_both_builds(case):
    specs, orc = batch(case)
    fixed = S.run(specs, planet())
    vs_oracle(fixed, specs, orc)
    generic = S.run(specs, planet(), generic=True)
    vs_oracle(generic, specs, orc)
    same_buffers(fixed, generic)
