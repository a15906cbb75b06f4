"""The table executor's kernels at the edges of the votes windows, the pending
capacities and the voter columns (tests/table_edges.py), bit for bit against
the restatements: order plane, release plane, nexec, status, stable clocks
and, from the _ps entry points, stable_sent; rows that are not written keep
their fill.  A stream that stops with FX_ERR_CAPACITY does so by construction:
each test names those streams and the event they stop at, asserts exactly that
list, and compares them with the restatement of the events before.  GPU only."""
import functools

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import table as ft

import table_edges as E
import table_ref as R
import table_ref_mk as RM
import table_ref_ps as RP
import table_shapes as T
import table_shapes_mk as TM
import table_shapes_ps as TP
from test_table_gpu import ORDER_TAG, compare as compare_sk
from test_table_mk_gpu import compare as compare_mk
from test_table_ps_gpu import compare as compare_ps

pytestmark = pytest.mark.gpu

ONCHIP, HBM = _lib.FX_TABLE_TIER_ONCHIP, _lib.FX_TABLE_TIER_HBM
CAPACITY = _lib.FX_ERR_CAPACITY
TOP = (1 << 32) - 1
# the entry points: single-key, multi-key (_mk), shards (_ps)
RUN = {"sk": R.run_stream, "mk": RM.run_stream, "ps": RP.run_stream}
COMPARE = {"sk": compare_sk, "mk": compare_mk, "ps": compare_ps}
VIA = {"sk": {}, "mk": dict(multi=True), "ps": dict(shards=True)}
ALL_MODES = ["sk", "mk", "ps"]


def fits_onchip(mode, ref):
    """The restatement says the stream stays inside the ONCHIP tier of that entry point."""
    if mode == "sk":
        return ref["max_pending"] <= _lib.FX_TABLE_ONCHIP_PENDING and ref["max_above"] <= _lib.FX_TABLE_ONCHIP_WINDOW
    fits = (ref["max_live"] <= _lib.FX_TABLE_MK_ONCHIP_LIVE and ref["max_stack"] <= _lib.FX_TABLE_MK_ONCHIP_STACK
            and ref["max_gap_above"] <= _lib.FX_TABLE_ONCHIP_WINDOW)
    return fits and (mode == "mk" or TP.fits_onchip(ref))


def first_over(mode, stream, n, thr, keys):
    """The event at which the stream leaves the ONCHIP tier: the shortest
    prefix whose restatement does not fit ends with it (what a stream asks of
    a tier only grows with its length)."""
    lo, hi = 0, len(stream)  # the prefix of lo events fits, the one of hi events does not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fits_onchip(mode, RUN[mode](stream[:mid], n, thr, keys)):
            lo = mid
        else:
            hi = mid
    return hi - 1


_refs = {}


def full_refs(name, mode, streams, n, thr, keys):
    """The restatement of whole streams, once per (stream set, entry point)."""
    if (name, mode) not in _refs:
        _refs[name, mode] = [RUN[mode](st, n, thr, keys) for st in streams]
    return _refs[name, mode]


def check(mode, streams, n, thr, keys, tier, stops=None, full=None):
    """One launch.  stops: {stream: the event it stops at with FX_ERR_CAPACITY};
    every other stream must equal its restatement (`full`, or computed here)."""
    stops = stops or {}
    refs = [E.stopped(RUN[mode], st, stops[s], n, thr, keys) if s in stops else
            full[s] if full is not None else RUN[mode](st, n, thr, keys) for s, st in enumerate(streams)]
    planes = ft.pack_table_streams(streams, n, keys)
    res = fd.run_table(planes, thr, order_fill=ORDER_TAG, tier=tier, **VIA[mode])
    assert [s for s in range(planes.S) if res.err[s] == CAPACITY] == sorted(stops)
    assert COMPARE[mode](planes, res, refs) == len(streams)
    return planes, res, refs


# ---- lifted streams: the generated streams above the first turn of the ring

@functools.lru_cache(maxsize=None)
def lifted(kind, B, chunk, count):
    """(streams, expected restatement results, n, thr, keys, entry point) of
    `count` generated streams lifted by B (None: so that the highest vote is
    2**32 - 1)."""
    n, thr = 5, T.quorum_sizes(5, 1, False)[2]
    if kind == "sk":
        keys, src, refs = T.KEYS, T.generated(n, 1, False, 50)[:count], T.generated_ref(n, 1, False, 50)[:count]
    elif kind == "mk":
        keys = TM.KEYS
        src, refs = TM.generated(n, 1, False, 2, 50)[:count], TM.generated_ref(n, 1, False, 2, 50)[:count]
    else:
        keys, groups = TP.KEYS, TP.generated(2, n, 1, 10)[:count // 2]
        src, refs = [st for g in groups for st in g[0]], [r for g in groups for r in g[2]]
    streams, want = [], []
    for st, ref in zip(src, refs):
        b = TOP - E.highest(st) if B is None else B
        up, pre = E.lift(list(st), b, n, keys, chunk)
        streams.append(up)
        want.append(E.lifted_ref(ref, b, pre))
    return streams, want, n, thr, keys


def lifted_full(kind, mode, B, chunk, count):
    """The restatement of the lifted streams themselves; its order, release,
    stable clocks (and stable_sent) are the unlifted ones moved."""
    streams, want, n, thr, keys = lifted(kind, B, chunk, count)
    full = full_refs(("lifted", kind, B, chunk, count), mode, streams, n, thr, keys)
    for got, w in zip(full, want):
        assert got["err"] == 0 and all(got[f] == w[f] for f in ("order", "release", "stable"))
    return streams, full, n, thr, keys


@pytest.mark.parametrize("B", [2028, 3 * 2048 - 20])
@pytest.mark.parametrize("tier,mode", [(ONCHIP, "sk"), (HBM, "sk"), (None, "sk"), (HBM, "mk"), (None, "mk"),
                                       (HBM, "ps"), (None, "ps")])
def test_lifted_single_key(B, tier, mode):
    """8 generated streams with every clock B higher, behind ranges of 2028 or
    2048 votes that walk the frontiers there: at 2028 no vote is 2048 above a
    frontier, at 3 * 2048 - 20 the ring has gone round twice.  Stops: in a
    fixed single-key ONCHIP launch every stream at event 0 (its first range is
    longer than that tier's window), nothing written; nowhere else."""
    streams, full, n, thr, keys = lifted_full("sk", mode, B, 2048, 8)
    assert max(r["max_above"] for r in full) == min(B, 2048)
    stops = {s: 0 for s in range(8)} if tier == ONCHIP else {}
    planes, res, _ = check(mode, streams, n, thr, keys, tier, stops, full)
    if tier == ONCHIP:
        assert np.all(res.nexec == 0)
    if tier is None:
        assert res.status == 0
        assert res.reruns == (8 if mode == "sk" else sum(not fits_onchip(mode, r) for r in full))


@pytest.mark.parametrize("B", [2028, 3 * 2048 - 20])
@pytest.mark.parametrize("tier", [ONCHIP, HBM, None])
@pytest.mark.parametrize("kind", ["mk", "ps"])
def test_lifted_multi_key_and_shards(kind, B, tier):
    """8 multi-key streams, and the two shard streams of one group, lifted as
    above.  The on-chip _mk / _ps kernels take the prefix (its ranges start at
    the frontier).  Stops: in a fixed ONCHIP launch exactly the streams whose
    restatement leaves that tier, at the event where it does; nowhere else."""
    streams, full, n, thr, keys = lifted_full(kind, kind, B, 2048, 8 if kind == "mk" else 2)
    over = [s for s, r in enumerate(full) if not fits_onchip(kind, r)]
    stops = {s: first_over(kind, streams[s], n, thr, keys) for s in over} if tier == ONCHIP else {}
    for s in over:  # what stops them is a gap beyond the window or the live ops: an event's own doing
        assert full[s]["max_stack"] <= _lib.FX_TABLE_MK_ONCHIP_STACK and full[s].get("max_buffered_pairs", 0) <= 64
    planes, res, _ = check(kind, streams, n, thr, keys, tier, stops, full)
    if tier is None:
        assert res.status == 0 and res.reruns == len(over)


@pytest.mark.parametrize("B", [5000, None])
@pytest.mark.parametrize("tier", [HBM, None])
@pytest.mark.parametrize("kind", ALL_MODES)
def test_lifted_by_one_range(kind, B, tier):
    """4 streams lifted by 5000, and so that their highest vote is 2**32 - 1,
    each frontier taken there by one range (voter, 1, B): such a range starts
    at the frontier and only moves it, on the HBM tier too.  No stream stops;
    the single-key ones all rerun (their ONCHIP kernel hands the range on)."""
    streams, full, n, thr, keys = lifted_full(kind, kind, B, None, 4)
    if B is None:
        assert all(E.highest(st) == TOP for st in streams)
    planes, res, _ = check(kind, streams, n, thr, keys, tier, {}, full)
    if tier is None:
        assert res.status == 0
        assert res.reruns == (4 if kind == "sk" else sum(not fits_onchip(kind, r) for r in full))


# ---- gappy streams: overlapping ranges, gaps up to the window, the ring wraps

@functools.lru_cache(maxsize=None)
def gappy_streams(win):
    return [E.gappy(seed, 3, 2, 1500 if win == 2048 else 600, win) for seed in range(8)]


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("win,tier", [(2048, HBM), (2048, None), (32, ONCHIP), (32, HBM), (32, None)])
def test_gappy(win, tier, mode):
    """8 streams whose ranges overlap earlier ones and reach exactly `win`
    above a frontier, past the third turn of the ring
    (test_table_edges_ref.py::test_gappy).  No stream stops in these launches;
    the driver reruns the ones the restatement puts beyond the ONCHIP tier."""
    streams = gappy_streams(win)
    full = full_refs(("gappy", win), mode, streams, 3, 2, 2)
    assert all(r["err"] == 0 and r["max_above"] == win for r in full)
    planes, res, _ = check(mode, streams, 3, 2, 2, tier, {}, full)
    if tier is None:
        over = sum(not fits_onchip(mode, r) for r in full)
        assert res.status == 0 and res.reruns == over == (8 if win == 2048 else 0)


# ---- a window filled to its last bit, and one vote beyond

EDGE_F = {32: [37], 2048: [2 * 2048 - 5, 3 * 2048 + 31]}


@pytest.mark.parametrize("mode", ["sk", "mk"])
def test_window_edge_onchip(mode):
    """W = 32, F = 37.  Stream 0 (the gap vote exactly 32 above the frontier)
    finishes; stream 1 (33 above) stops at its gap-vote event, and the driver
    finishes it on HBM."""
    (a, _), (b, gap) = E.window_edge(37, 32, 0), E.window_edge(37, 32, 1)
    check(mode, [a, b], 3, 2, 1, ONCHIP, {1: gap})
    planes, res, _ = check(mode, [a, b], 3, 2, 1, None)
    assert res.status == 0 and res.reruns == 1


@pytest.mark.parametrize("mode", ["sk", "mk"])
@pytest.mark.parametrize("tier", [HBM, None])
def test_window_edge_hbm(mode, tier):
    """Streams 0-1: W = 32, gap vote at and beyond the on-chip window.  2-3:
    W = 2048 at F = 2 * 2048 - 5 (the walk crosses the ring's end) and
    3 * 2048 + 31 (it starts on a word's last bit), gap vote exactly 2048
    above.  4-5: the same with the gap vote 2049 above: they stop at the
    gap-vote event, and HBM is the last tier.  6: stream 0 again, complete
    beside them."""
    built = [E.window_edge(37, 32, 0), E.window_edge(37, 32, 1)]
    built += [E.window_edge(F, 2048, over) for over in (0, 1) for F in EDGE_F[2048]]
    built.append(E.window_edge(37, 32, 0))
    streams = [st for st, _ in built]
    planes, res, refs = check(mode, streams, 3, 2, 1, tier, {4: built[4][1], 5: built[5][1]})
    assert res.nexec.tolist() == [1, 1, 1, 1, 0, 0, 1]
    if tier is None:
        full = [RUN[mode](st, 3, 2, 1) for st in streams]
        assert res.status == CAPACITY and res.reruns == sum(not fits_onchip(mode, r) for r in full) == 5


@pytest.mark.parametrize("mode", ["sk", "mk"])
@pytest.mark.parametrize("tier,F,W", [(ONCHIP, 37, 32), (HBM, 37, 32), (HBM, 2 * 2048 - 5, 2048)])
def test_seen_inside(tier, F, W, mode):
    """Ranges wholly above the frontier and wholly seen before: each of the
    three streams stops at its last event with FX_ERR_VOTE_RANGE (the
    restatement says so), its earlier rows and stable clocks complete.  No
    capacity stops."""
    streams = E.seen_inside(F, W)
    planes, res, refs = check(mode, streams, 3, 2, 1, tier)
    assert res.err.tolist() == [_lib.FX_ERR_VOTE_RANGE] * 3 and res.nexec.tolist() == [1, 1, 1]
    assert res.stable_clock.tolist() == [[1]] * 3


# ---- pending ops at the capacities, all leaving in one event

@pytest.mark.parametrize("mode", ALL_MODES)
def test_mass_onchip(mode):
    """64 pending ops fill the ONCHIP tier and leave in one event; of 65
    (stream 1) the 65th attached event, row 64, stops the stream."""
    streams = [E.mass(64, 3, 1), E.mass(65, 3, 2)]
    planes, res, _ = check(mode, streams, 3, 2, 1, ONCHIP, {1: 64})
    assert res.nexec.tolist() == [64, 0]
    planes, res, _ = check(mode, streams[:1], 3, 2, 1, None)
    assert res.status == 0 and res.reruns == 0
    planes, res, _ = check(mode, streams, 3, 2, 1, None)
    assert res.status == 0 and res.reruns == 1 and res.nexec.tolist() == [64, 65]


@pytest.mark.parametrize("mode", ALL_MODES)
def test_mass_hbm(mode):
    """64, 65 and 512 ops (all eight register rows of every lane, equal clocks
    with different dots across rows) leave in one event in (clock, dot) order;
    of 513 (stream 3) the 513th attached event, row 512, stops the stream, in
    a fixed HBM launch and in the driver."""
    streams = [E.mass(64, 3, 1), E.mass(65, 3, 2), E.mass(512, 3, 3), E.mass(513, 3, 4)]
    planes, res, refs = check(mode, streams, 3, 2, 1, HBM, {3: 512})
    assert res.nexec.tolist() == [64, 65, 512, 0]
    ids = [(streams[2][a][3], streams[2][a][2]) for a in refs[2]["order"]]
    assert len(ids) == 512 and ids == sorted(ids)
    planes, res, _ = check(mode, streams[2:], 3, 2, 1, None, {1: 512})
    assert res.status == CAPACITY and res.reruns == 2 and res.nexec.tolist() == [512, 0]


# ---- the voter columns: n = 1, 2 and 16; 64 ranges in an event

@pytest.mark.parametrize("tier", [ONCHIP, HBM, None])
@pytest.mark.parametrize("n,fq,thr", [(16, 11, 9), (16, 16, 16), (16, 2, 1), (1, 1, 1), (2, 2, 1)])
def test_n_at_its_ends(n, fq, thr, tier):
    """8 generated streams at the ends of the voter columns; the restatement
    keeps them on chip, so no stream stops in any launch."""
    streams = [ft.synth_table_streams(seed, n, fq, 8, 40, 50, 6, 4) for seed in range(8)]
    full = full_refs(("n", n, fq, thr), "sk", streams, n, thr, 8)
    assert all(r["err"] == 0 and fits_onchip("sk", r) for r in full)
    planes, res, _ = check("sk", streams, n, thr, 8, tier, {}, full)
    assert planes.vmax == fq and np.all(res.nexec == 40)
    if tier is None:
        assert res.status == 0 and res.reruns == 0


@pytest.mark.parametrize("tier", [ONCHIP, HBM])
def test_max_votes_in_one_event(tier):
    """FX_TABLE_MAX_VOTES = 64 ranges in one event, four per voter of n = 16
    (lane 15 included); beside it the same event with the 64th a repeat:
    FX_ERR_VOTE_RANGE, nothing stored.  No capacity stops."""
    streams = [E.max_votes_event(), E.max_votes_event(repeat=True)]
    planes, res, _ = check("sk", streams, 16, 16, 1, tier)
    assert planes.vmax == 64 and res.err.tolist() == [0, _lib.FX_ERR_VOTE_RANGE]
    assert res.nexec.tolist() == [1, 0] and res.stable_clock.tolist() == [[2], [0]]


# ---- key rows

def on_keys(stream, key_map):
    return [ev[:1] + (key_map.get(ev[1], ev[1]),) + tuple(ev[2:]) for ev in stream]


def test_the_last_onchip_key():
    """Exactly FX_TABLE_ONCHIP_KEYS keys, and the last of them in the fourth
    stream of a workgroup (the end of its LDS).  No stream stops."""
    keys = _lib.FX_TABLE_ONCHIP_KEYS
    streams = [ft.synth_table_streams(seed, 3, 2, keys, 40, 30, 6, 4) for seed in range(4)]
    streams[3] = on_keys(streams[3], {0: keys - 1, keys - 1: 0})
    assert sum(ev[1] == keys - 1 for ev in streams[3]) > 10
    planes, res, refs = check("sk", streams, 3, 2, keys, ONCHIP)
    assert np.all(res.nexec == 40) and refs[3]["stable"][keys - 1] > 5


def test_a_thousand_keys_on_hbm():
    """1,000 key rows in `state`, the first and the last in use.  No stream stops."""
    streams = [on_keys(ft.synth_table_streams(seed, 3, 2, 2, 40, 50, 6, 4), {1: 999}) for seed in range(2)]
    planes, res, refs = check("sk", streams, 3, 2, 1000, HBM)
    assert np.all(res.nexec == 40) and all(r["stable"][0] > 5 and r["stable"][999] > 5 for r in refs)
