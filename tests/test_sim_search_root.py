"""The executor's search in the all-on-chip simulator (k_sim) where it is
decided at the root: a first Add whose first unexecuted dep is not pending is
filed under that dep without a search; a walk starts at the root's first
unexecuted dep and, in the compiled-in builds for n <= 5, jumps over the
executed deps of each vertex, so a retried waiter whose deps are all executed
is popped as a singleton SCC in its first step (or filed again under its first
unexecuted dep).  Orders, counters and histograms must stay what the reference
computes.

Each case is computed once on the simulator oracle, run on the compiled-in
geometry build and on the run-time geometry build (generic=True), compared to
the oracle (orders, fast / slow / stable, events, trace, end time, latency
sums, the three histograms; the checks of test_sim_gpu.run_and_compare, on the
shared oracle output), and the two builds buffer by buffer.  No tolerances.
GCP regions, EPaxos n = 5 f = 2 unless said:

  chain        1 client per region, 30 commands, conflicts {50, 100} %, seed
               41: first Adds filed under a missing dep, retries that execute
               as singletons, values of up to n + 1 = 6 deps with executed ones
               between unexecuted ones (the compiled-in build's walk)
  two_clients  2 clients per region, 20 commands, {10, 100} %, seed 42 (10
               clients: the run-time build's tables): roots whose first
               unexecuted dep is itself pending, so a walk starts past the
               skipped deps; SCCs of 2 and more; several waiters released by
               one dot, in ascending order; a waiter retried that still misses
               another dep (the epoch mark)
  two_keys     two_clients with 2 keys per command from a pool of 4, {50,
               100} %, seed 43: values of more than 4 deps, a parent that
               continues after a child SCC
  atlas_n7, atlas_n3  the cases of test_sim_slot_row (and its oracle outputs):
               the other compiled-in geometries

test_oracle_shapes_are_what_they_claim checks the claims on the oracle's
output.  chain and two_keys also run under the register fills of
test_sim_poison.  Which search paths each case takes, counted by the profile
build, is recorded in profiles/sim_search_root.md.
"""
import numpy as np
import pytest

from fantoch_amd import sim as S
from oracle import oracle_lib as O
from test_sim_gpu import planet, to_oracle
from test_sim_percmd_paths import max_chain, same_buffers, vs_oracle
from test_sim_poison import FILLS, poisoner
from test_sim_slot_row import oracle as slot_row_oracle


def _chain():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, commands_per_client=30, conflict_rate=c, seed=41, instance=i)
            for i, c in enumerate([50, 100])]


def _two_clients():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, clients_per_region=2, commands_per_client=20, conflict_rate=c,
                   seed=42, instance=i) for i, c in enumerate([10, 100])]


def _two_keys():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, clients_per_region=2, commands_per_client=20, conflict_rate=c,
                   keys_per_command=2, pool_size=4, seed=43, instance=i) for i, c in enumerate([50, 100])]


CASES = {"chain": _chain, "two_clients": _two_clients, "two_keys": _two_keys}
ALL_CASES = sorted(CASES) + ["atlas_n3", "atlas_n7"]
_ORACLE = {}


def oracle(case):
    """(specs, oracle outputs) of a case, computed once and shared (read only)."""
    if case not in CASES:
        return slot_row_oracle(case)
    if case not in _ORACLE:
        specs = CASES[case]()
        orc = O.sim_batch([to_oracle(s) for s in specs], threads=8)
        assert all(o["status"] == 0 for o in orc)
        _ORACLE[case] = (specs, orc)
    return _ORACLE[case]


def test_oracle_shapes_are_what_they_claim():
    """On the oracle's output (not the GPU's): commands wait for deps
    (ExecutionDelay non-zero), SCCs of 2 and more in two_clients and two_keys,
    of 3 and more in one of them."""
    longest = {}
    for case in sorted(CASES):
        specs, orc = oracle(case)
        for s, o in zip(specs, orc):
            delayed = int(o["delay"][1:].sum())
            print("%s %d %%: singletons %d, chains >= 2: %d, longest %d, delayed executions %d of %d, slow paths %d"
                  % (case, s.conflict_rate, o["chain"][1], o["chain"][2:].sum(), max_chain(o), delayed,
                     o["delay"].sum(), o["slow"].sum()))
            assert delayed > 0
            assert s.commands_per_client <= 30 and s.clients_per_region * 5 <= 10
        if case != "chain":
            assert sum(int(o["chain"][2:].sum()) for o in orc) > 0
        longest[case] = max(max_chain(o) for o in orc)
    assert max(longest["two_clients"], longest["two_keys"]) >= 3
    # chain: most commands execute alone, after waiting (filed under a dep, retried)
    specs, orc = oracle("chain")
    assert all(o["chain"][1] > 0 for o in orc)
    specs, orc = oracle("two_keys")
    for s in specs:
        assert s.keys_per_command == 2
    for s, o in zip(specs, orc):
        cap = O.sim_capture_raw(to_oracle(s))
        nd = max(int(cap["nd"][p, :int(cap["len"][p])].max()) for p in range(5))
        print("two_keys %d %%: longest value %d deps" % (s.conflict_rate, nd))
        assert nd > 4


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL_CASES)
def test_search_paths_match_the_oracle_on_both_builds(case):
    specs, orc = oracle(case)
    fixed = S.run(specs, planet())
    vs_oracle(fixed, specs, orc)
    generic = S.run(specs, planet(), generic=True)
    vs_oracle(generic, specs, orc)
    same_buffers(fixed, generic)


@pytest.mark.gpu
@pytest.mark.parametrize("case,generic", [("chain", False), ("chain", True), ("two_keys", False)])
def test_poisoned_registers_do_not_change_the_searches(case, generic):
    specs, orc = oracle(case)
    for mode, tag in FILLS:
        res = S.run(specs, planet(), generic=generic, before_launch=poisoner(mode, tag))
        try:
            vs_oracle(res, specs, orc)
        except AssertionError as e:
            raise AssertionError("fill (%d, %#x): %s" % (mode, tag, e))
