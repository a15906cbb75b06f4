"""The capacity-rerun driver (fx::run_ladder) behind fx_table_run, fx_pending_run
and fx_pred_run: batches of 300 streams, so the collector of the streams to
rerun runs a second 256-thread block, with every third stream over the first
tier, so it compacts inside every wavefront.  The reruns reach the next tier in
the collector's order, not ascending: every stream must still come out as it
does alone.  Each batch repeats a handful of distinct streams round-robin, so
a restatement runs once per distinct stream.  GPU only."""
import functools

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import streams as fs
from fantoch_amd import table as ft
from oracle import oracle_lib as O

import pending_shapes as PS
import pred_shapes as P
import table_ref as R
import table_shapes as T
from test_pending_gpu import same_bytes
from test_table_gpu import ORDER_TAG, compare

pytestmark = pytest.mark.gpu

S = 300
OVER = [s for s in range(S) if s % 3 == 0]
DUP, BAD = 7, 260  # the streams the status cases break: both fit the first tier


def picks(n_over, n_fit):
    """Stream s of the batch -> its distinct stream: the over ones first, each kind round-robin."""
    out, k = [], 0
    for s in range(S):
        if s % 3 == 0:
            out.append((s // 3) % n_over)
        else:
            out.append(n_over + k % n_fit)
            k += 1
    return out


def tiled(arr, small_S, steps, pick):
    """arr: planes of a batch of small_S streams; the same planes of the batch of its streams `pick`."""
    sp, bp = _lib.plane_words(small_S, steps), _lib.plane_words(len(pick), steps)
    rows = np.arange(steps)
    src = np.stack([_lib.index(rows, d, steps) for d in pick])
    dst = np.stack([_lib.index(rows, s, steps) for s in range(len(pick))])
    out = np.zeros(len(arr) // sp * bp, arr.dtype)
    for j in range(len(arr) // sp):
        out[j * bp + dst] = arr[j * sp + src]
    return out


# ------------------------------------------------------------------ table
N, F, TINY = 5, 1, False


def tile_table(small, pick):
    """The streams `pick` of the packed batch `small` as a batch of their own."""
    big = ft.TablePlanes(len(pick), small.steps, small.n, small.keys, small.vmax,
                         lengths=small.lengths[np.array(pick)].copy())
    for name in ("hdr", "dot", "clock", "votes"):
        setattr(big, name, tiled(getattr(small, name), small.S, small.steps, pick))
    return big


@functools.lru_cache(maxsize=None)
def table_case():
    """The six streams of test_table_gpu.test_escalation, their restatements, and two broken copies of a
    fitting stream: one with its first command repeated (a repeated dot), one with an invalid header word."""
    fq, _, thr = T.quorum_sizes(N, F, TINY)
    streams = [ft.synth_table_streams(seed, N, fq, T.KEYS, 150, 100, 80, 4) for seed in range(3)]
    streams += [list(st) for st in T.generated(N, F, TINY, 10)[:3]]
    refs = [R.run_stream(st, N, thr, T.KEYS) for st in streams]
    over = [r["max_pending"] > _lib.FX_TABLE_ONCHIP_PENDING or r["max_above"] > _lib.FX_TABLE_ONCHIP_WINDOW
            for r in refs]
    assert over == [True] * 3 + [False] * 3
    assert all(r["max_pending"] <= _lib.FX_TABLE_HBM_PENDING and r["max_above"] <= _lib.FX_TABLE_HBM_WINDOW
               for r in refs)
    first = next(i for i, ev in enumerate(streams[4]) if ev[0] == "A")
    dup = streams[4][:first + 1] + streams[4][first:]
    small = ft.pack_table_streams(streams + [dup, streams[5]], N, T.KEYS)
    small.hdr[_lib.index(0, 7, small.steps)] = ft.table_hdr(_lib.FX_TABLE_DETACHED, 0, 0xFFFFFF)  # no such key
    return small, refs, thr


@functools.lru_cache(maxsize=None)
def table_run():
    """The healthy batch through fx_table_run, once for both tests (nobody writes to it)."""
    small, refs, thr = table_case()
    planes = tile_table(small, picks(3, 3))
    return planes, fd.run_table(planes, thr, order_fill=ORDER_TAG)


def test_table_reruns_every_third_stream():
    small, refs, thr = table_case()
    planes, res = table_run()
    assert res.reruns == len(OVER) == 100 and res.status == 0
    assert compare(planes, res, [refs[d] for d in picks(3, 3)]) == S


def test_status_is_the_lowest_failing_streams():
    small, refs, thr = table_case()
    alone = fd.run_table(small, thr, tier=_lib.FX_TABLE_TIER_HBM).err  # one launch, every stream by itself
    assert list(alone[:6]) == [0] * 6 and alone[6] != alone[7]
    assert all(int(e) not in (0, _lib.FX_ERR_CAPACITY) for e in alone[6:])
    pick = picks(3, 3)
    pick[DUP], pick[BAD] = 6, 7
    planes = tile_table(small, pick)
    res = fd.run_table(planes, thr, order_fill=ORDER_TAG)
    assert res.status == alone[6] and res.err[DUP] == alone[6] and res.err[BAD] == alone[7]
    assert res.reruns == 100 and np.count_nonzero(res.err) == 2
    # the other streams as in the healthy batch
    _, healthy = table_run()
    good = [s for s in range(S) if s not in (DUP, BAD)]
    rows = np.concatenate([_lib.index(np.arange(planes.steps), s, planes.steps) for s in good])
    assert np.array_equal(res.order[rows], healthy.order[rows])
    assert np.array_equal(res.release[rows], healthy.release[rows])
    assert np.array_equal(res.nexec[good], healthy.nexec[good])
    assert np.array_equal(res.stable_clock[good], healthy.stable_clock[good])


# ------------------------------------------------------------------ pending
def pending_case(broken=False):
    sts = [PS.stream(PS.live(65 if s % 3 == 0 else 64)) for s in range(S)]
    if broken:
        sts[DUP] = PS.stream(PS.singles(5, 100) + [(PS.rifl(7), 9)] + PS.singles(5, 200))  # a count of 9
        sts[BAD] = dict(PS.stream(PS.live(64)), nexec=131)                                 # nexec beyond steps
    return PS.Case("ladder", sts, steps=130)


def run_pending(case):
    return fd.run_pending(case.order, case.nexec, case.rifl, case.count, case.S, case.steps, case.count_mask,
                          case.process, fill=0xA5)


def test_pending_reruns_every_third_stream():
    case = pending_case()
    dev = run_pending(case)
    assert dev.reruns == 100 and dev.status == 0 and not np.any(dev.err)
    same_bytes(dev, case.run_host(None))


def test_pending_returns_its_own_status():
    case = pending_case(broken=True)
    dev = run_pending(case)  # (a refused call raises)
    assert dev.status == 0 and dev.reruns == 100
    assert dev.err[DUP] == PS.E and dev.err[BAD] == PS.O and np.count_nonzero(dev.err) == 2
    same_bytes(dev, case.run_host(None))


# ------------------------------------------------------------------ pred
def test_pred_reruns_through_both_tiers():
    wide = P.random_streams(3, 2, 2, 110, keys=3, reverse_pct=80)  # test_pred_gpu.test_very_wide_deps' shape
    small, *clocks = P.pack_pred_streams(wide + [P.SIMPLE], 2)
    pick = picks(2, 1)
    planes = fs.Planes(S, small.steps, small.dmax, small.n, lengths=small.lengths[np.array(pick)].copy(),
                       **{name: tiled(getattr(small, name), small.S, small.steps, pick) for name in ("dot", "hdr", "deps")})
    clo, chi, nd = (tiled(c, small.S, small.steps, pick) for c in clocks)
    assert planes.dmax > 200
    res = fd.run_pred(planes, clo, chi, ndeps=nd)
    o_order, o_rel, o_nexec, o_err = O.pred_batch_execute(planes, clo, chi, threads=8, ndeps=nd)
    assert res.status == 0 and not np.any(o_err)
    assert np.array_equal(res.err, o_err) and np.array_equal(res.nexec, o_nexec)
    for s in range(S):
        rows = _lib.index(np.arange(int(o_nexec[s])), s, planes.steps)
        assert np.array_equal(res.order[rows], o_order[rows]), "order differs on stream %d" % s
    # a fixed tier that does not take the shape writes no status (the 0xAB sentinel stays)
    capacity = 0
    for tier in (_lib.FX_PRED_TIER_SMALL, _lib.FX_PRED_TIER_LDS):
        one = fd.run_pred(planes, clo, chi, ndeps=nd, tier=tier)
        assert one.status in (0, _lib.FX_ERR_UNSUPPORTED)
        capacity += int(np.count_nonzero(one.err == _lib.FX_ERR_CAPACITY))
    assert res.reruns == capacity and res.reruns >= 100
