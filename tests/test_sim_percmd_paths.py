"""The per-command bookkeeping of the all-on-chip simulator (k_sim) that lives
in lanes: the log cursors (execution log, dot -> client table, latency log:
one lane predicate and a vector store per entry), the executors' clocks
(AEClock::add on the owning lane), the ExecutionDelay counts, the small set
operations of key_deps.add_cmd and QuorumDeps, and the workload's key draws.
Each case is computed once on the simulator oracle, run on the compiled-in
geometry build and on the run-time geometry build (generic=True), compared to
the oracle as test_sim_gpu does (orders, fast / slow / stable, events, trace,
end time, latency sums, the three histograms), and the two builds buffer by
buffer.

GCP regions, EPaxos n = 5 f = 2 unless said:

  one_client   1 client per region, 30 commands, conflicts {0, 1, 50, 99,
               100} %, seed 21: delays at and past 256 ms (the global-bin path
               of the delay histogram), chains up to 5, slow paths; 1 and 99 %
               run the RNG draw, 0 and 100 % skip it
  two_clients  2 clients per region, 20 commands, {0, 10, 100} %, seed 22 (10
               clients: the run-time build only): executions out of their
               source's sequence order (the clock's window case and its
               multi-bit frontier jump), chains up to 10
  two_keys     two_clients with 2 keys per command from a pool of 4, {10, 50,
               100} %, a 64-bit seed with the top bit set and instance numbers
               past 2^40: both modulos of the draw, two-key add_cmd with
               duplicate candidates
  atlas_n3     Atlas n = 3 f = 1, 30 commands, {2, 100} %, seed 23: threshold
               QuorumDeps, chains of 2

test_oracle_exercises_the_paths checks those claims on the oracle's output.
The log-cap tests rerun one_client with logs shorter than what is produced,
without a latency log, and with histograms narrower than the samples.
"""
import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import sim as S
from oracle import oracle_lib as O
from test_sim_gpu import assert_instance_parity, planet, to_oracle


def _one_client():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, commands_per_client=30, conflict_rate=c, seed=21, instance=i)
            for i, c in enumerate([0, 1, 50, 99, 100])]


def _two_clients():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, clients_per_region=2, commands_per_client=20, conflict_rate=c,
                   seed=22, instance=i) for i, c in enumerate([0, 10, 100])]


def _two_keys():
    regs = planet().ids(S.GCP5[:5])
    return [S.spec(S.EPAXOS, 5, 2, regs, regs, clients_per_region=2, commands_per_client=20, conflict_rate=c,
                   keys_per_command=2, pool_size=4, seed=2**63 + 12345, instance=2**40 + i)
            for i, c in enumerate([10, 50, 100])]


def _atlas_n3():
    regs = planet().ids(S.GCP5[:3])
    return [S.spec(S.ATLAS, 3, 1, regs, regs, commands_per_client=30, conflict_rate=c, seed=23, instance=i)
            for i, c in enumerate([2, 100, 2, 100])]


CASES = {"one_client": _one_client, "two_clients": _two_clients, "two_keys": _two_keys, "atlas_n3": _atlas_n3}
_ORACLE = {}


def oracle(case):
    """(specs, oracle outputs) of a case, computed once and shared (read only)."""
    if case not in _ORACLE:
        specs = CASES[case]()
        orc = O.sim_batch([to_oracle(s) for s in specs], threads=8)
        assert all(o["status"] == 0 for o in orc)
        _ORACLE[case] = (specs, orc)
    return _ORACLE[case]


def out_of_order(o, n):
    """Executions that reach a process's clock out of their source's sequence
    order: (past the frontier + 1: AEClock::add's window case, frontier moves
    of more than one: the window's run of set bits joins the frontier)."""
    window = jumps = 0
    for order in o["executed"]:
        front = [0] * (n + 1)
        above = [set() for _ in range(n + 1)]
        for d in order:
            src, sq = int(d) >> 24, int(d) & 0xFFFFFF
            if sq == front[src] + 1:
                f = sq
                while f + 1 in above[src]:
                    above[src].discard(f + 1)
                    f += 1
                jumps += f > sq
                front[src] = f
            elif sq > front[src]:
                above[src].add(sq)
                window += 1
    return window, jumps


def max_chain(o):
    return int(np.flatnonzero(o["chain"]).max())


def test_oracle_exercises_the_paths():
    """The cases' claims, on the oracle's output (not the GPU's)."""
    specs, orc = oracle("one_client")
    by_rate = {s.conflict_rate: o for s, o in zip(specs, orc)}
    o50 = by_rate[50]
    print("one_client 50 %%: delays >= 256: %d, in [64, 256): %d, longest chain %d"
          % (o50["delay"][256:].sum(), o50["delay"][64:256].sum(), max_chain(o50)))
    assert o50["delay"][256:].sum() > 0 and o50["delay"][64:256].sum() > 0 and max_chain(o50) >= 3
    for r in (99, 100):
        o = by_rate[r]
        print("one_client %d %%: delays >= 256: %d, longest chain %d, slow paths %d"
              % (r, o["delay"][256:].sum(), max_chain(o), o["slow"].sum()))
        assert o["delay"][256:].sum() > 0 and max_chain(o) >= 5 and o["slow"].sum() > 0
    # the draw: rates strictly between 0 and 100 run it, and it decides both ways
    # somewhere in the 1 % / 99 % instances (the host restatement of the workload)
    assert set(by_rate) == {0, 1, 50, 99, 100}
    kinds = {(r, S.command(s, c, k)[0][0] == 0) for s in specs for r in [s.conflict_rate] if r in (1, 50, 99)
             for c in range(1, 6) for k in range(30)}
    print("one_client draws (rate, conflicted):", sorted(kinds))
    assert (50, True) in kinds and (50, False) in kinds and (1, False) in kinds and (99, True) in kinds

    specs, orc = oracle("two_clients")
    by_rate = {s.conflict_rate: o for s, o in zip(specs, orc)}
    w, j = out_of_order(by_rate[10], 5)
    print("two_clients 10 %%: out-of-order executions %d, multi-bit frontier jumps %d" % (w, j))
    assert w > 0 and j > 0
    o = by_rate[100]
    print("two_clients 100 %%: longest chain %d, delays >= 256: %d" % (max_chain(o), o["delay"][256:].sum()))
    assert max_chain(o) >= 10 and o["delay"][256:].sum() > 0

    specs, orc = oracle("two_keys")
    for s, o in zip(specs, orc):
        assert s.seed >> 63 == 1 and s.instance >> 40 == 1
        w, j = out_of_order(o, 5)
        cmds = [S.command(s, c, k)[0] for c in range(1, 11) for k in range(20)]
        pool = sum(k < 4 for ks in cmds for k in ks)
        print("two_keys %d %%: out-of-order %d, jumps %d, slow paths %d, pool keys %d of %d"
              % (s.conflict_rate, w, j, o["slow"].sum(), pool, 2 * len(cmds)))
        assert w > 0 and o["slow"].sum() > 0 and pool > 0
        assert all(len(ks) == 2 and ks[0] < ks[1] for ks in cmds)

    specs, orc = oracle("atlas_n3")
    for s, o in zip(specs, orc):
        if s.conflict_rate == 100:
            print("atlas_n3 100 %%: longest chain %d, fast %d, slow %d" % (max_chain(o), o["fast"].sum(), o["slow"].sum()))
            assert max_chain(o) >= 2 and o["fast"].sum() + o["slow"].sum() > 0


def hists_vs_oracle(res, orc):
    """The batch histograms against the oracle's, folded into the run's bins
    (a sample past the last bin counts in it)."""
    def fold(h, bins):
        h = np.asarray(h, np.uint64)
        if h.shape[-1] <= bins:
            return np.pad(h, [(0, 0)] * (h.ndim - 1) + [(0, bins - h.shape[-1])])
        return np.concatenate([h[..., :bins - 1], h[..., bins - 1:].sum(axis=-1, keepdims=True)], axis=-1)
    assert np.array_equal(res.latency_hist, fold(sum(o["latency"] for o in orc), res.latency_hist.shape[1]))
    assert np.array_equal(res.chain, fold(sum(o["chain"] for o in orc), res.chain.shape[0]))
    assert np.array_equal(res.delay, fold(sum(o["delay"] for o in orc), res.delay.shape[0]))


def vs_oracle(res, specs, orc):
    bad = [(i, int(e)) for i, e in enumerate(res.err) if e]
    assert not bad, "instances failed: %s" % bad[:8]
    assert res.reruns == 0
    for i, (s, o) in enumerate(zip(specs, orc)):
        assert_instance_parity(res, i, s, o)
    hists_vs_oracle(res, orc)


def same_buffers(a, b):
    assert np.array_equal(a.executed_len, b.executed_len)
    assert np.array_equal(a._executed, b._executed)
    assert np.array_equal(a._dot_client, b._dot_client)
    assert (a._lat is None and b._lat is None) or np.array_equal(a._lat, b._lat)
    assert np.array_equal(a.stats, b.stats)
    assert np.array_equal(a.latency_hist, b.latency_hist)
    assert np.array_equal(a.chain, b.chain)
    assert np.array_equal(a.delay, b.delay)
    assert np.array_equal(a.err, b.err)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_percmd_paths_match_the_oracle_on_both_builds(case):
    specs, orc = oracle(case)
    fixed = S.run(specs, planet())
    vs_oracle(fixed, specs, orc)
    generic = S.run(specs, planet(), generic=True)
    vs_oracle(generic, specs, orc)
    same_buffers(fixed, generic)


_FULL = {}


def full_run():
    """one_client with logs that hold everything (checked against the oracle),
    the reference of the capped runs' dot -> client and latency rows: the
    oracle reports latencies as histograms and names no clients."""
    if not _FULL:
        specs, orc = oracle("one_client")
        res = S.run(specs, planet())
        vs_oracle(res, specs, orc)
        # one client per region, in the processes' regions: client p + 1 submits process p + 1's dots
        for i in range(len(specs)):
            want = np.zeros((5, res.exec_cap), np.uint32)
            want[:, :30] = np.arange(1, 6, dtype=np.uint32)[:, None]
            assert np.array_equal(res._dot_client[i], want)
        _FULL["res"] = res
    return _FULL["res"]


def counters_vs_oracle(res, specs, orc):
    """What a run with short or absent logs still reports in full."""
    assert not res.err.any() and res.reruns == 0
    for i, (s, o) in enumerate(zip(specs, orc)):
        assert [int(x) for x in res.executed_len[i]] == [len(e) for e in o["executed"]]
        assert [int(x) for x in res.fast(i)] == [int(x) for x in o["fast"]]
        assert [int(x) for x in res.slow(i)] == [int(x) for x in o["slow"]]
        assert [int(x) for x in res.stable(i)] == [int(x) for x in o["stable"]]
        assert (res.end_ms(i), res.events(i), res.trace(i)) == (o["end_ms"], o["events"], o["trace"])
    hists_vs_oracle(res, orc)


@pytest.mark.gpu
@pytest.mark.parametrize("generic", [False, True])
def test_logs_shorter_than_the_run(generic):
    """exec_cap = 16 and lat_cap = 7, both smaller than what a run produces
    (some 150 executions and 30 own dots per process, 30 latencies per client): every row is the
    prefix of that length, nothing is written past it, and executed_len still
    counts everything."""
    specs, orc = oracle("one_client")
    full = full_run()
    res = S.run(specs, planet(), exec_cap=16, lat_cap=7, generic=generic)
    counters_vs_oracle(res, specs, orc)
    assert res._executed.shape[2] == 16 and res._lat.shape[2] == 7
    for i, o in enumerate(orc):
        for p in range(5):
            assert len(o["executed"][p]) > 16
            assert np.array_equal(res._executed[i, p], o["executed"][p][:16])
        assert np.array_equal(res._dot_client[i], full._dot_client[i][:, :16])
        assert np.array_equal(res._dot_client[i], np.repeat(np.arange(1, 6, dtype=np.uint32)[:, None], 16, axis=1))
        assert np.array_equal(res.latencies(i), full.latencies(i)[:, :7])


@pytest.mark.gpu
@pytest.mark.parametrize("generic", [False, True])
def test_no_latency_log(generic):
    specs, orc = oracle("one_client")
    full = full_run()
    res = S.run(specs, planet(), lat_cap=0, generic=generic)
    counters_vs_oracle(res, specs, orc)
    assert res._lat is None
    assert np.array_equal(res._executed, full._executed)
    assert np.array_equal(res._dot_client, full._dot_client)
    assert np.array_equal(res.stats, full.stats)


@pytest.mark.gpu
@pytest.mark.parametrize("generic", [False, True])
def test_histograms_narrower_than_the_samples(generic):
    """delay_bins = 64 and chain_bins = 4: samples past the last bin are
    clamped into it, where they are counted directly and at the flush."""
    specs, orc = oracle("one_client")
    full = full_run()
    res = S.run(specs, planet(), delay_bins=64, chain_bins=4, generic=generic)
    assert sum(o["delay"] for o in orc)[64:].sum() > 0 and sum(o["chain"] for o in orc)[4:].sum() > 0
    counters_vs_oracle(res, specs, orc)
    assert res.delay.shape[0] == 64 and res.chain.shape[0] == 4
    assert np.array_equal(res._executed, full._executed)
    assert np.array_equal(res._lat, full._lat)
