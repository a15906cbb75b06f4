"""GPU predecessors executor (fantoch_amd/csrc/pred_exec.hip: k_pred,
fx_pred_execute, fx_pred_run) on the edge cases of pred_edges, bit for bit
against the restatement (pred_ref) at each tier's limits: every byte of
order, release, nexec and err over buffers of 0xA5 bytes (the kernel never
stores FX_RELEASE_NONE: a row that never executes keeps the fill), the
ladder's reruns and status, and the ExecutionDelay histogram.  GPU only; the
pair conditions and the oracle are in test_pred_edges_ref.py."""
import numpy as np
import pytest

import pred_edges as E
import pred_ref as R
from fantoch_amd import _lib
from fantoch_amd import device as fd

pytestmark = pytest.mark.gpu

CASES = E.all_cases()
NBINS = 4096
FIXED = [(c, t, a) for c in CASES for t in c.tiers for a in (False, True)]
LADDER = [(c, a) for c in CASES for a in (False, True)]


def launch(case, tier, at_commit=False, stream_map=None):
    planes, clo, chi, nd = case.packed()
    return fd.run_pred(planes, clo, chi, ndeps=None if case.header_nd else nd, execute_at_commit=at_commit, tier=tier,
                       nbins_delay=NBINS, stream_map=stream_map, fill=E.FILL)


def check_delay(case, res, want):
    hist = E.delay_hist(case.packed()[0], want["order"], want["release"], want["nexec"], NBINS)
    assert np.array_equal(res.delay, hist), "%s: ExecutionDelay differs at bin %d" % (
        case.name, int(np.flatnonzero(res.delay != hist)[0]))


@pytest.mark.parametrize("case,tier,at_commit", FIXED,
                         ids=["%s at %s%s" % (c.name, R.TIER_NAME[t], " at commit" * a) for c, t, a in FIXED])
def test_fixed_tier_equals_restatement_at_its_limits(gpu, case, tier, at_commit):
    res = launch(case, tier, at_commit)
    assert res.status == 0
    want = case.expected(tier, at_commit)
    case.check(res, want)
    check_delay(case, res, want)
    if not at_commit:
        for p in case.pairs:  # err exact per stream: 0 for the fitting half, FX_ERR_CAPACITY for the other
            assert p.tier == tier and (res.err[p.fit], res.err[p.exceed]) == (0, _lib.FX_ERR_CAPACITY)
    if case.hand and not at_commit:
        for s in range(case.S):
            rows = _lib.index(np.arange(2), s, case.packed()[0].steps)
            assert [int(x) & 0x7FFFFFFF for x in res.order[rows]] == case.hand[s], "stream %d" % s


@pytest.mark.parametrize("case,at_commit", LADDER, ids=["%s%s" % (c.name, " at commit" * a) for c, a in LADDER])
def test_ladder_equals_unbounded_restatement(gpu, case, at_commit):
    """fx_pred_run: every stream's result is that of the last tier it ran at -- the unbounded one unless HBM
    stops it too -- and the reruns are the ones the per-tier restatements predict."""
    res = launch(case, None, at_commit)
    want, reruns, status = case.expected_ladder(at_commit)
    case.check(res, want)
    assert (res.reruns, res.status) == (reruns, status)
    check_delay(case, res, want)
    for s in range(case.S):
        r, u = case.laddered(s, at_commit)[0], case.restated(s, None, at_commit)
        if r["err"] != _lib.FX_ERR_CAPACITY:
            assert (r["order"], r["release"], r["err"]) == (u["order"], u["release"], u["err"]), "stream %d" % s
    if case.pairs and R.HBM not in case.tiers and not at_commit:
        assert np.all(res.err == 0) and res.reruns >= 1


BY = {c.name: c for c in CASES}


@pytest.mark.parametrize("name,tier", [("lengths", R.SMALL), ("lengths", R.LDS), ("lengths", R.HBM),
                                       ("lengths compiled", R.SMALL), ("lanes compiled 41", R.SMALL),
                                       ("many", R.SMALL), ("errors", R.HBM)])
def test_stream_map_covers_a_subset(gpu, name, tier):
    """Lane l of the launch runs stream stream_map[l] (HBM: on the l-th tables); the other streams keep 0xA5."""
    case = BY[name]
    for chosen in (list(range(case.S))[::-1], [s for s in range(case.S) if s % 3 == 1][::-1], [case.S - 1]):
        res = launch(case, tier, stream_map=chosen)
        assert res.status == 0 and res.delay is None
        case.check(res, case.expected(tier, only=set(chosen)))


def test_an_error_leaves_the_tile_alone(gpu):
    case = BY["tile error"]
    res = launch(case, R.SMALL)
    assert [int(s) for s in np.flatnonzero(res.err)] == [37] and res.err[37] == _lib.FX_ERR_DOT_RANGE
    case.check(res, case.expected(R.SMALL))
