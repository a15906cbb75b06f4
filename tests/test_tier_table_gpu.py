"""The tier table's max_deps at work: a batch whose widest Add has more deps than
its first tier reads starts at FX_TIER_LDS_LARGE instead, and the drop-in
handle's pending set decodes from a wide-HBM block.  Three batches of 128
streams (two 64-stream tiles, so the split tier would see more than one) of 40
Adds at n = 5; Add WIDE_AT of every stream names the 9, 15 or 17 dots before
it, one more than the lane-register, wave and group tiers read.  The oracle runs
once per batch.  GPU only."""
import ctypes
import functools

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import streams as fs
from fantoch_amd.executor import GraphExecutor
from oracle import oracle_lib

from test_gpu_parity import release_rows, valid_rows

pytestmark = pytest.mark.gpu

S, ROWS, N, WIDE_AT = 128, 40, 5, 30
LDS_LARGE, GLOBAL = 1, 2


def stream(seed, width):
    """40 Adds over 5 sources: up to 3 deps among the 6 dots before, every ninth Add waits for the next dot
    of another source (pending until that source issues again), Add WIDE_AT names the `width` dots before it."""
    rng = np.random.default_rng(seed)
    seqs, issued, out = [0] * N, [], []
    for i in range(ROWS):
        src = int(rng.integers(N))
        seqs[src] += 1
        recent = issued[-6:]
        k = min(len(recent), int(rng.integers(0, 4)))
        deps = [recent[j] for j in rng.choice(len(recent), size=k, replace=False)] if k else []
        if i % 9 == 4:
            other = (src + 1) % N
            deps.append((other + 1, seqs[other] + 1))
        if i == WIDE_AT:
            deps = issued[-width:]
        out.append(((src + 1, seqs[src]), deps, i))
        issued.append(out[-1][0])
    return out


@functools.lru_cache(maxsize=None)
def batch(width):
    planes = fs.pack_streams([stream(1000 * width + s, width) for s in range(S)], N)
    assert planes.dmax == width and planes.S == S
    return planes, oracle_lib.batch_execute(planes, threads=8)


@pytest.mark.parametrize("width,first", [(9, _lib.FX_TIER_LANE_REG), (15, _lib.FX_TIER_WAVE),
                                         (17, _lib.FX_TIER_GROUP), (17, None)])
def test_too_wide_for_the_first_tier_starts_at_lds_large(gpu, width, first):
    planes, (o_order, o_rel, o_nexec, o_err) = batch(width)
    res = fd.run_batch(planes, tier=first, metrics=False)
    first = _lib.FX_TIER_DEFAULT if first is None else first
    assert res.tier_counts[first] == 0
    assert res.tier_counts[LDS_LARGE] == S
    # bit-exact parity, as test_gpu_parity.assert_parity
    assert np.array_equal(res.err, o_err), (np.unique(res.err), np.unique(o_err))
    assert np.array_equal(res.nexec, o_nexec)
    rows = valid_rows(res.order, res.nexec, planes.S, planes.steps)
    assert np.array_equal(res.order[rows], o_order[rows])
    rrows = release_rows(planes.lengths, planes.S, planes.steps)
    assert np.array_equal(res.release[rrows], o_rel[rrows])


def test_handle_pending_decodes_a_wide_hbm_block(gpu):
    """The log of test_gpu_parity.test_executor_many_pending_escalates_to_hbm_tables, cut where the
    oracle's pending set first passes the slots of FX_TIER_GLOBAL: the smallest log that moves the
    handle to the HBM tables, whose saved block fx_graph_executor_pending then decodes."""
    info = _lib.TierInfo()
    assert gpu.fx_tier_query(GLOBAL, N, ctypes.byref(info)) == _lib.FX_OK
    p = fs.synth_params(seed=5, instances=1, n=5, cmds=640, window=320, cycle_pct=30, conflicts=(100,), clients=64)
    ex = GraphExecutor(1, 0, N, monitor=True)
    g = oracle_lib.Graph(1, N)
    for dot, deps, t, _kind in fs.synth_host(p).stream(0):
        ex.handle_add(dot, dot, [0], deps, t)
        g.handle_add(dot, deps, t)
        want = g.pending(cap=256)
        if len(want) > info.pending_cap:
            break
    assert len(want) == info.pending_cap + 1
    assert ex.pending() == sorted(want)
    assert [d for d, _ in ex.drain_dots()] == [d for d, _, _ in g.drain()]
