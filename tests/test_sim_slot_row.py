"""The dot-table slot as a lane row in the all-on-chip simulator (k_sim): a
handler looks its dot up once, reads the slot with one LDS read by lanes and
takes every header field from that row; an MCommit hands the slot to the
executor, which stores the committed and the executed count of SL_MASKS in one
word, or frees the slot, without a second look-up.

Each case is computed once on the simulator oracle, run on the compiled-in
geometry build and on the run-time geometry build (generic=True), compared to
the oracle (orders, fast / slow / stable, events, trace, end time, latency
sums, the three histograms), and the two builds buffer by buffer.  GCP
regions, one client per region and one key per command unless said:

  epaxos_n5    EPaxos n = 5 f = 2, 30 commands, conflicts {0, 50, 100} %,
               seed 31: the singleton path (committed and executed count in
               one store), the fifth executing process freeing the slot (150
               dots through 40 slots), slow paths (MConsensus / MConsensusAck
               on the row), chains >= 3 (SCC members through remembered slots)
  two_clients  2 clients per region, 20 commands, {10, 100} %, seed 32 (10
               clients: the run-time build only): chains up to 10, waiters
               released through check_pending / try_pending, 200 dots through
               64 slots while other vertices are pending
  two_keys     two_clients with 2 keys per command from a pool of 4, {50,
               100} %, seed 33: slots of 41 words, committed values of more
               than 4 deps, acks of up to 2 K = 4 deps, chains >= 3
  atlas_n7     Atlas n = 7 f = 2 over 7 regions, 30 commands, {10, 100} %,
               seed 34: the n = 7 compiled-in build, threshold QuorumDeps,
               state bytes in both SL_PST words (p >= 4)
  atlas_n3     Atlas n = 3 f = 1, 30 commands, {2, 100} %, seed 35: the
               coordinator's own MCollect -> own MCollectAck on one slot

test_oracle_exercises_the_paths checks those claims on the oracle's output.
The 256-slot tier reruns a lagging-replica placement of test_sim_gpu's
capacity test with 30 clients, which holds more than 128 live dots (slot
indices past 64), and epaxos_n5 / two_keys run under the register poisoning of
test_sim_poison: a row lane the kernel never wrote must not change a result.
"""
import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import sim as S
from oracle import oracle_lib as O
from test_sim_gpu import planet, run_and_compare, to_oracle
from test_sim_percmd_paths import max_chain, same_buffers, vs_oracle
from test_sim_poison import FILLS, poisoner


def _epaxos_n5():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, commands_per_client=30, conflict_rate=c, seed=31, instance=i)
            for i, c in enumerate([0, 50, 100])]


def _two_clients():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, clients_per_region=2, commands_per_client=20, conflict_rate=c,
                   seed=32, instance=i) for i, c in enumerate([10, 100])]


def _two_keys():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, clients_per_region=2, commands_per_client=20, conflict_rate=c,
                   keys_per_command=2, pool_size=4, seed=33, instance=i) for i, c in enumerate([50, 100])]


def _atlas_n7():
    regs = list(range(0, 14, 2))  # 7 of the planet's regions
    return [S.spec(S.ATLAS, 7, 2, regs, regs, commands_per_client=30, conflict_rate=c, seed=34, instance=i)
            for i, c in enumerate([10, 100])]


def _atlas_n3():
    regs = planet().ids(S.GCP5[:3])
    return [S.spec(S.ATLAS, 3, 1, regs, regs, commands_per_client=30, conflict_rate=c, seed=35, instance=i)
            for i, c in enumerate([2, 100])]


CASES = {"epaxos_n5": _epaxos_n5, "two_clients": _two_clients, "two_keys": _two_keys, "atlas_n7": _atlas_n7,
         "atlas_n3": _atlas_n3}
_ORACLE = {}


def oracle(case):
    """(specs, oracle outputs) of a case, computed once and shared (read only)."""
    if case not in _ORACLE:
        specs = CASES[case]()
        orc = O.sim_batch([to_oracle(s) for s in specs], threads=8)
        assert all(o["status"] == 0 for o in orc)
        _ORACLE[case] = (specs, orc)
    return _ORACLE[case]


def dots(o):
    """The distinct dots an instance executed anywhere, and those every process executed."""
    sets = [set(int(d) for d in e) for e in o["executed"]]
    return set.union(*sets), set.intersection(*sets)


def test_oracle_exercises_the_paths():
    """The cases' claims, on the oracle's output (not the GPU's)."""
    specs, orc = oracle("epaxos_n5")
    by_rate = {s.conflict_rate: o for s, o in zip(specs, orc)}
    for r, o in by_rate.items():
        anywhere, everywhere = dots(o)
        print("epaxos_n5 %d %%: singletons %d, longest chain %d, slow paths %d, dots %d (executed by all 5: %d)"
              % (r, o["chain"][1], max_chain(o), o["slow"].sum(), len(anywhere), len(everywhere)))
        # 40 slots: a dot's slot is freed by its fifth execution and taken again
        assert o["chain"][1] > 0 and len(everywhere) > 40
    assert max_chain(by_rate[0]) == 1 and by_rate[0]["slow"].sum() == 0
    assert max_chain(by_rate[50]) >= 3 and max_chain(by_rate[100]) >= 3
    assert by_rate[50]["slow"].sum() > 0 and by_rate[100]["slow"].sum() > 0

    specs, orc = oracle("two_clients")
    by_rate = {s.conflict_rate: o for s, o in zip(specs, orc)}
    for r, o in by_rate.items():
        anywhere, everywhere = dots(o)
        print("two_clients %d %%: longest chain %d, chains > 1: %d, dots %d (by all 5: %d)"
              % (r, max_chain(o), o["chain"][2:].sum(), len(anywhere), len(everywhere)))
        # 64 slots for 200 dots, and SCCs of more than one dot: vertices wait
        # while slots are freed and taken again
        assert len(everywhere) > 64 and o["chain"][2:].sum() > 0
    assert max_chain(by_rate[100]) >= 10

    specs, orc = oracle("two_keys")
    for s, o in zip(specs, orc):
        cap = O.sim_capture_raw(to_oracle(s))
        nd = max(int(cap["nd"][p, :int(cap["len"][p])].max()) for p in range(5))
        print("two_keys %d %%: longest value %d deps, longest chain %d, slow paths %d"
              % (s.conflict_rate, nd, max_chain(o), o["slow"].sum()))
        assert s.keys_per_command == 2 and nd > 4 and max_chain(o) >= 3 and o["slow"].sum() > 0

    specs, orc = oracle("atlas_n7")
    for s, o in zip(specs, orc):
        anywhere, everywhere = dots(o)
        print("atlas_n7 %d %%: longest chain %d, fast %s, slow %s, dots by all 7: %d"
              % (s.conflict_rate, max_chain(o), list(o["fast"]), list(o["slow"]), len(everywhere)))
        # every process coordinates (its state byte is written by h_submit's
        # MCollect to itself), processes 5-7 use the second SL_PST word
        assert all(int(f) + int(w) > 0 for f, w in zip(o["fast"], o["slow"])) and len(everywhere) > 32
    assert max_chain(orc[1]) >= 2

    specs, orc = oracle("atlas_n3")
    for s, o in zip(specs, orc):
        print("atlas_n3 %d %%: longest chain %d, fast %d, slow %d"
              % (s.conflict_rate, max_chain(o), o["fast"].sum(), o["slow"].sum()))
        assert o["fast"].sum() + o["slow"].sum() == 90  # every command through its coordinator's own ack
    assert max_chain(orc[1]) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_slot_row_paths_match_the_oracle_on_both_builds(case):
    specs, orc = oracle(case)
    fixed = S.run(specs, planet())
    vs_oracle(fixed, specs, orc)
    generic = S.run(specs, planet(), generic=True)
    vs_oracle(generic, specs, orc)
    same_buffers(fixed, generic)


def _lagging_replica():
    """One of the placements of test_sim_gpu.test_capacity_escalation_is_exact
    (a replica in Asia lags the four others), with 6 clients per region."""
    regs = planet().ids(sorted(["asia-east1", "europe-west1", "europe-west2", "europe-west4", "us-east4"]))
    return [S.spec(S.ATLAS, 5, 1, regs, regs, clients_per_region=6, commands_per_client=20, conflict_rate=c,
                   seed=9, instance=i) for i, c in enumerate((2, 50))]


@pytest.mark.gpu
def test_slot_indices_past_64_in_the_256_slot_tier():
    """More than 128 dots are live at once in these instances: with 128 dot
    slots (and a message pool that cannot be what overflows) they stop with
    FX_ERR_SIM_CAPACITY.  The dot table hands out its lowest free slot, so the
    rerun of fx_sim_run_tiered on the 256-slot tables (four slot words per
    lane) uses slot indices past 64 and past 128: they travel from h_mcommit
    to the executor, and every output equals the oracle's."""
    specs = _lagging_replica()
    small = S.run(specs, planet(), dot_slots=128, ring_entries=4096, tiered=False)
    sites = [int(x) for x in small.stats[:, _lib.FX_SIM_STAT_ERR_SITE]]
    print("128 slots: err %s at source lines %s" % ([int(e) for e in small.err], sites))
    assert all(int(e) == _lib.FX_ERR_SIM_CAPACITY for e in small.err)
    res, _ = run_and_compare(specs)
    print("reruns at the larger tables: %d for %d instances" % (res.reruns, len(specs)))
    assert res.reruns > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["epaxos_n5", "two_keys"])
@pytest.mark.parametrize("generic", [False, True])
def test_poisoned_registers_do_not_change_the_rows(case, generic):
    specs, orc = oracle(case)
    for mode, tag in FILLS:
        res = S.run(specs, planet(), generic=generic, before_launch=poisoner(mode, tag))
        try:
            vs_oracle(res, specs, orc)
        except AssertionError as e:
            raise AssertionError("fill (%d, %#x): %s" % (mode, tag, e))
