"""GPU table executor with multi-key commands (fx_table_run_mk /
fx_table_execute_mk) against the CPU restatement (tests/table_ref_mk.py), bit
for bit: order plane, release plane, nexec, status and the stable clocks; rows
the executor does not write stay at their fill.  GPU only."""
import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import table as ft

import table_ref as R
import table_ref_mk as RM
import table_shapes as T
import table_shapes_mk as TM

pytestmark = pytest.mark.gpu

ORDER_TAG = 0xA5
ORDER_TAG_WORD = 0xA5A5A5A5
ONCHIP, HBM = _lib.FX_TABLE_TIER_ONCHIP, _lib.FX_TABLE_TIER_HBM


def compare(planes, res, refs, allow_capacity=False):
    """Every stream against its restatement; with allow_capacity a stream may
    instead have stopped with FX_ERR_CAPACITY.  Returns the streams compared.
    Rows beyond nexec (order) and rows of detached events, of partials not
    executed and beyond the stream's length (release) must be untouched."""
    done = 0
    for s, ref in enumerate(refs):
        orows = _lib.index(np.arange(planes.steps), s, planes.steps)
        if allow_capacity and res.err[s] == _lib.FX_ERR_CAPACITY:
            continue
        done += 1
        assert res.err[s] == ref["err"], "status differs on stream %d" % s
        assert res.nexec[s] == ref["nexec"], "nexec differs on stream %d" % s
        want = np.full(planes.steps, ORDER_TAG_WORD, np.uint32)
        want[:ref["nexec"]] = np.array(ref["order"], np.uint32) | np.uint32(_lib.FX_ORDER_SCC_START)
        assert np.array_equal(res.order[orows], want), "order differs on stream %d" % s
        rel = np.full(planes.steps, _lib.FX_RELEASE_NONE, np.uint32)
        for a, step in ref["release"].items():
            rel[a] = step
        assert np.array_equal(res.release[orows], rel), "release differs on stream %d" % s
        assert list(res.stable_clock[s]) == ref["stable"], "stable clocks differ on stream %d" % s
    return done


def run(streams, n, thr, keys, refs=None, allow_capacity=False, **kw):
    planes = ft.pack_table_streams(streams, n, keys)
    res = fd.run_table(planes, thr, order_fill=ORDER_TAG, **kw)
    if refs is None:
        refs = [RM.run_stream(st, n, thr, keys, execute_at_commit=kw.get("execute_at_commit", False))
                for st in streams]
    done = compare(planes, res, refs, allow_capacity)
    return planes, res, refs, done


@pytest.mark.parametrize("tier", [None, ONCHIP, HBM])
def test_hand_written_many_copies(tier):
    """The hand-written streams, 11 copies of each in one launch (66 streams:
    more than one plane tile), against the orders written out by hand."""
    names = sorted(TM.HAND) * 11
    streams = [list(TM.HAND[nm][0]) for nm in names]
    planes, res, refs, done = run(streams, TM.HAND_N, TM.HAND_THR, TM.HAND_KEYS, tier=tier)
    assert planes.nkeys is not None and done == len(names) == 66 and np.all(res.err == 0)
    for s, nm in enumerate(names):
        _, order, release, _ = TM.HAND[nm]
        rows = _lib.index(np.arange(planes.steps), s, planes.steps)
        assert res.nexec[s] == len(order)
        assert [int(x) & 0x7FFFFFFF for x in res.order[rows][:len(order)]] == order
        got = {a: int(res.release[rows][a]) for a in range(len(streams[s])) if res.release[rows][a] != _lib.FX_RELEASE_NONE}
        assert got == release
    if tier is None:
        assert res.status == 0 and res.reruns == 0


@pytest.mark.parametrize("tier", [None, ONCHIP, HBM])
@pytest.mark.parametrize("n,f,tiny,kmax,conflict",
                         [cfg + (k, c) for cfg in TM.CONFIGS for k in TM.KMAX for c in TM.CONFLICTS])
def test_generated_streams(tier, n, f, tiny, kmax, conflict):
    """24 streams of about 120 commands with 1..kmax keys over 16 keys, ragged
    lengths, steps not a multiple of 4 (a stream that was cut short keeps
    partials waiting in the queues); a fixed tier may stop a stream with
    FX_ERR_CAPACITY and the on-chip tier must finish more than half.

    Lag 2 and window 2 were chosen on the CPU with the restatement: over the
    16 configurations the streams need at most 6 live ops and a to_executors
    of 4, far inside FX_TABLE_MK_ONCHIP_LIVE / _STACK = 64; what stops a stream
    on chip is a vote more than FX_TABLE_ONCHIP_WINDOW = 32 above its voter's
    frontier in a range that does not start at the frontier (max_gap_above),
    which happens in no stream at 0 and 10 % conflicts and in at most 3 of 24
    at 50 and 100 % (with lag 4, window 3: up to 13 of 24)."""
    thr = T.quorum_sizes(n, f, tiny)[2]
    streams = [list(st) for st in TM.generated(n, f, tiny, kmax, conflict)]
    refs = list(TM.generated_ref(n, f, tiny, kmax, conflict))
    for s, cut in ((1, 5), (5, 13), (11, 22)):  # cut three short: their references are not the shared ones
        streams[s] = streams[s][:len(streams[s]) - cut]
        refs[s] = RM.run_stream(streams[s], n, thr, TM.KEYS)
    longest = max(range(len(streams)), key=lambda s: len(streams[s]))
    if len(streams[longest]) % 4 == 0:
        streams[longest] = streams[longest] + [("D", 0, [])]  # an event without votes
        refs[longest] = RM.run_stream(streams[longest], n, thr, TM.KEYS)
    fits = sum(r["max_live"] <= _lib.FX_TABLE_MK_ONCHIP_LIVE and r["max_stack"] <= _lib.FX_TABLE_MK_ONCHIP_STACK
               and r["max_gap_above"] <= _lib.FX_TABLE_ONCHIP_WINDOW for r in refs)
    assert fits > len(streams) // 2
    planes, res, refs, done = run(streams, n, thr, TM.KEYS, refs=refs, allow_capacity=tier is not None, tier=tier)
    assert planes.steps % 4 != 0 and len(set(planes.lengths.tolist())) > 3
    if tier is None:
        assert res.status == 0 and done == planes.S
    if tier == ONCHIP:
        assert done == fits > planes.S // 2
    if tier == HBM:
        assert done == planes.S


def test_generated_70_streams_ragged_tile():
    n, f, tiny = 5, 1, False
    thr = T.quorum_sizes(n, f, tiny)[2]
    streams = [list(st) for st in TM.generated(n, f, tiny, 3, 10, count=70, cmds=40)]
    streams[69] = streams[69][:-3]
    planes, res, refs, done = run(streams, n, thr, TM.KEYS)
    assert planes.S == 70 and done == 70 and res.status == 0


def test_escalation():
    """A long lag at 100 % conflicts: the restatement says the streams need
    more than the on-chip tier holds, so they stop there and rerun on HBM
    with the restatement's results."""
    n, f, tiny = 5, 1, False
    fq, _, thr = T.quorum_sizes(n, f, tiny)
    streams = [ft.synth_table_streams_mk(seed, n, fq, TM.KEYS, 150, 100, 80, 4, 2) for seed in range(3)]
    streams += [list(st) for st in TM.generated(n, f, tiny, 2, 10)[:3]]
    refs = [RM.run_stream(st, n, thr, TM.KEYS) for st in streams]
    over = [r["max_live"] > _lib.FX_TABLE_MK_ONCHIP_LIVE or r["max_gap_above"] > _lib.FX_TABLE_ONCHIP_WINDOW
            for r in refs]
    assert over == [True] * 3 + [False] * 3
    assert all(r["max_live"] <= _lib.FX_TABLE_MK_HBM_LIVE and r["max_above"] <= _lib.FX_TABLE_HBM_WINDOW for r in refs)
    planes, res, refs, done = run(streams, n, thr, TM.KEYS, refs=refs)
    assert res.reruns == 3 and res.status == 0 and done == 6
    one = fd.run_table(planes, thr, tier=ONCHIP)
    assert one.err.tolist() == [_lib.FX_ERR_CAPACITY] * 3 + [0] * 3


def test_more_live_ops_than_the_onchip_tier():
    """70 two-key commands that wait on their first key: 70 live ops are more
    than FX_TABLE_MK_ONCHIP_LIVE; then their second keys arrive."""
    n, thr, keys = 3, 2, 2
    st = [TM.att(0, (1, i + 1), i + 1, i + 1, 2) for i in range(70)]
    st += [TM.att(1, (1, i + 1), i + 1, i + 1, 2) for i in range(70)]
    ref = RM.run_stream(st, n, thr, keys)
    assert ref["max_live"] == 71 and ref["nexec"] == 140
    planes, res, refs, done = run([st, st[:60] + st[70:130]], n, thr, keys)
    assert res.reruns == 1 and res.status == 0 and done == 2
    one = fd.run_table(planes, thr, tier=ONCHIP)
    assert one.err.tolist() == [_lib.FX_ERR_CAPACITY, 0]


@pytest.mark.parametrize("tier", [ONCHIP, HBM])
def test_execute_at_commit(tier):
    streams = [list(st) for st in TM.generated(5, 1, False, 3, 10)[:5]] + [list(TM.HAND["chain"][0])]
    planes, res, refs, done = run(streams, 5, 3, TM.KEYS, execute_at_commit=True, tier=tier)
    assert done == 6 and np.all(res.stable_clock == 0)
    assert all(r["nexec"] == sum(ev[0] == "A" for ev in st) for r, st in zip(refs, streams))


@pytest.mark.parametrize("tier", [None, HBM])
def test_errors_beside_good_streams(tier):
    X, Y, S1, att = TM.X, TM.Y, TM.S1, TM.att
    good = list(TM.HAND["chain"][0])
    streams = [
        good,
        [att(0, X, 1, 1, 2), att(1, X, 1, 1, 3)] + good,                      # another nkeys for the dot
        [att(0, X, 1, 1, 2), att(2, S1, 1, 1, 1), att(0, X, 1, 2, 2)] + good,  # the key again
        [att(0, X, 1, 1, 2), att(1, X, 2, 1, 2)] + good,                      # another clock
        # a bad vote range in the middle of a command: the rows of events 0 and 1 stay
        [att(0, X, 1, 1, 2), att(2, S1, 1, 1, 1), ("A", 1, X, 1, [(1, 1, 1), (1, 1, 1)], 2)] + good,
        [att(0, X, 1, 1, 9)] + good,                                         # nkeys beyond FX_TABLE_MAX_CMD_KEYS
        [att(0, X, 1, 1, 0)] + good,
        # a third event of a two-key command while its first partial waits for its message
        [att(0, Y, 1, 1, 2), att(2, X, 2, 1, 2), att(0, X, 2, 2, 2), att(1, Y, 1, 1, 2), att(1, X, 2, 2, 2)],
        good,
    ]
    planes, res, refs, done = run(streams, TM.HAND_N, TM.HAND_THR, TM.HAND_KEYS, tier=tier)
    assert done == len(streams)
    bad = _lib.FX_ERR_INVALID_ARG
    assert res.err.tolist() == [0, bad, bad, bad, _lib.FX_ERR_VOTE_RANGE, bad, bad, bad, 0]
    assert res.nexec.tolist() == [4, 0, 1, 0, 1, 0, 0, 3, 4]
    if tier is None:
        assert res.status == bad and res.reruns == 0


@pytest.mark.parametrize("tier", [None, ONCHIP, HBM])
def test_single_key_streams_equal_the_single_key_entry_points(tier):
    """Streams of single-key commands through the _mk entry points (an nkeys
    plane of ones) give exactly what fx_table_run / fx_table_execute give."""
    n, f, tiny = 5, 2, False
    thr = T.quorum_sizes(n, f, tiny)[2]
    # (streams inside the on-chip tier of the single-key kernel: the _mk kernel takes longer vote ranges there)
    streams = [list(st) for st, ref in zip(T.generated(n, f, tiny, 10), T.generated_ref(n, f, tiny, 10))
               if ref["max_pending"] <= _lib.FX_TABLE_ONCHIP_PENDING and ref["max_above"] <= _lib.FX_TABLE_ONCHIP_WINDOW]
    assert len(streams) > 12
    streams[3] = streams[3][:-7]
    streams.append(T.kat_stream("majority", T.KAT["majority"]["stepwise"]) * 2)  # FX_ERR_DOUBLE_INDEX
    planes = ft.pack_table_streams(streams, n, T.KEYS)
    assert planes.nkeys is None
    old = fd.run_table(planes, thr, order_fill=ORDER_TAG, tier=tier)
    new = fd.run_table(planes, thr, order_fill=ORDER_TAG, tier=tier, multi=True)
    for field in ("order", "release", "nexec", "err", "stable_clock"):
        assert np.array_equal(getattr(old, field), getattr(new, field)), field
    assert (old.status, old.reruns) == (new.status, new.reruns)
    assert np.count_nonzero(old.err) == 1 and old.nexec.sum() > 12 * T.CMDS
    refs = [R.run_stream(st, n, thr, T.KEYS) for st in streams]
    assert compare(planes, new, refs) == len(streams)
