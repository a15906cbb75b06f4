"""The cut driver (fantoch_amd/csrc/graph_cut.hip, fx_batch_run_cut) on the
edge cases of cut_edges: every byte of order, release, nexec and err over
buffers of 0xA5, and the stats against cut_ref.  GPU only; that the cases sit
on their limits is shown in test_cut_edges_ref.py.

The outputs of a wrong cut come out right all the same -- a stream whose
segments do not all execute completely is run again whole -- so what tells is
failed_streams == 0 and segments, single_segments, max_segment and
whole_streams, each equal to what cut_ref predicts from the planes alone.  The
batch slots show in tier_counts at the tier the segment batch starts on
(Case.first_tier); the sum over the tiers is the same number only where no
segment is run again one tier up (Case.reruns_possible), and with a double dot
in the batch the count depends on which store of its position came last.
The call's status is that of its lowest stream with one, FX_OK in every case
without a stopped stream (Case.status).  nexec and err equal the tiered
driver's on the same planes, but for the stream whose sparse seqs lie above
every tier's window (Case.beyond_tiered): the tiered driver must end that one
in FX_ERR_CAPACITY, the cut driver must equal the oracle.  Before every launch
the register file is filled with garbage (test_sim_poison).

Measured on an MI355X: every case of test_cut_at_the_limits under 1 s (the
64-chunk cases 0.8 s, MAX_SEG 0.5 s), the stale-scratch test 1.0 s,
test_cut_rounds 3.2 s, of which fx_batch_run_cut with its copies 0.08 s."""
import time

import numpy as np
import pytest

import cut_edges as E
from fantoch_amd import _lib
from fantoch_amd import device as fd
from test_gpu_parity import assert_parity, oracle_hists
from test_sim_poison import FILLS, poisoner

pytestmark = pytest.mark.gpu

CASES = E.all_cases()
BY = {c.name: c for c in CASES}
STATS = ("segments", "single_segments", "max_segment", "whole_streams")


def run_cut(case, fill=0):
    return fd.run_batch(case.planes(), cut=True, order_fill=E.FILL, execute_at_commit=case.at_commit,
                        before_launch=poisoner(*FILLS[fill % len(FILLS)]))


def stats_of(res):
    st = res.cut_stats
    return {name: int(getattr(st, name)) for name in STATS + ("failed_streams",)}


def check(case, res):
    planes, a = case.planes(), case.analysis()
    want, left = case.want()
    assert res.status == case.status()
    if not case.stops():
        assert res.status == _lib.FX_OK
        assert_parity(planes, res, execute_at_commit=case.at_commit)
    for name in E.NAMES:  # every word: a cut stream's rows, and 0xA5 outside them
        got, exp = getattr(res, name), want[name]
        if name == "release" and len(left):
            got, exp = got.copy(), exp.copy()
            got[left] = exp[left] = 0
        assert np.array_equal(got, exp), "%s: %s differs at word %d" % (case.name, name,
                                                                        int(np.flatnonzero(got != exp)[0]))
    ref = fd.run_batch(planes, metrics=False, execute_at_commit=case.at_commit)  # the tiered driver
    same = np.ones(planes.S, bool)
    same[list(case.beyond_tiered)] = False  # sparse seqs: past every tier's window, not past the cut driver
    assert np.all(ref.err[~same] == _lib.FX_ERR_CAPACITY) and not np.any(ref.err[same] == _lib.FX_ERR_CAPACITY)
    assert np.array_equal(res.nexec[same], ref.nexec[same]) and np.array_equal(res.err[same], ref.err[same])
    got = stats_of(res)
    print("%s: %s tier_counts %s" % (case.name, got, list(res.cut_stats.tier_counts)[:_lib.FX_NUM_TIERS]))
    assert got["failed_streams"] == 0
    counts = list(res.cut_stats.tier_counts)
    if a.sparse or case.at_commit:  # through run_tiered at once: the stats stay zeroed
        assert all(got[name] == 0 for name in STATS) and sum(counts) == 0
        return
    assert {name: got[name] for name in STATS} == a.stats()
    assert got["single_segments"] <= got["segments"]
    if not a.racy:
        assert counts[case.first_tier()] == a.slots
        if not a.slots or not case.reruns_possible():
            assert sum(counts) == a.slots
    if case.hists:
        order, release, nexec, _ = case.oracle()
        chain, delay = oracle_hists(planes, order, release, nexec, 64, 4096)
        assert np.array_equal(res.chain, chain) and np.array_equal(res.delay, delay)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cut_at_the_limits(gpu, case):
    check(case, run_cut(case, fill=len(case.name)))


def test_cut_rounds(gpu):
    """steps = 2^20 + 1025: the carry between the rounds of k_chunk_excl_blk, in the max scan (the flags) and in
    the sum scans (segment ids, class offsets).  Five planes of 268 MB: the time is copies, not kernels."""
    case = E.rounds_case()
    t0 = time.time()
    res = run_cut(case)
    print("rounds: run_batch %.2f s" % (time.time() - t0))
    check(case, res)


def test_small_batch_after_a_large_one_reads_no_stale_scratch(gpu):
    """The driver's buffers are scratch slots that persist, are reused and are not cleared (rk, seg_*, bidx,
    sg.*): MAX_SEG, then one short stream, then MAX_SEG again in one process, every time the same results."""
    big, small = BY["MAX_SEG"], BY["streams S=1"]
    first = run_cut(big)
    check(big, first)
    check(small, run_cut(small, fill=1))
    again = run_cut(big, fill=2)
    check(big, again)
    for name in E.NAMES + ("chain", "delay"):
        assert np.array_equal(getattr(first, name), getattr(again, name)), name
    assert stats_of(first) == stats_of(again)
    assert list(first.cut_stats.tier_counts) == list(again.cut_stats.tier_counts)
