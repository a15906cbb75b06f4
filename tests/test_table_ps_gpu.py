"""GPU table executor over several shards (fx_table_run_ps /
fx_table_execute_ps) against the CPU restatement (tests/table_ref_ps.py), bit
for bit: order plane, release plane, stable_sent plane, nexec, status and the
stable clocks; rows the executor does not write stay at their fill.  GPU only."""
from collections import Counter

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import table as ft

import table_ref_ps as RP
import table_shapes as T
import table_shapes_mk as TM
import table_shapes_ps as TP

pytestmark = pytest.mark.gpu

ORDER_TAG = 0xA5
ORDER_TAG_WORD = 0xA5A5A5A5
ONCHIP, HBM = _lib.FX_TABLE_TIER_ONCHIP, _lib.FX_TABLE_TIER_HBM


def compare(planes, res, refs, allow_capacity=False):
    """Every stream against its restatement; with allow_capacity a stream may
    instead have stopped with FX_ERR_CAPACITY.  Returns the streams compared.
    Rows beyond nexec (order), rows of events that executed nothing (release),
    rows of events that did not make a command stable at the shard
    (stable_sent) and rows beyond the stream's length must be untouched."""
    done = 0
    assert res.stable_sent is not None
    for s, ref in enumerate(refs):
        rows = _lib.index(np.arange(planes.steps), s, planes.steps)
        if allow_capacity and res.err[s] == _lib.FX_ERR_CAPACITY:
            continue
        done += 1
        assert res.err[s] == ref["err"], "status differs on stream %d" % s
        assert res.nexec[s] == ref["nexec"], "nexec differs on stream %d" % s
        want = np.full(planes.steps, ORDER_TAG_WORD, np.uint32)
        want[:ref["nexec"]] = np.array(ref["order"], np.uint32) | np.uint32(_lib.FX_ORDER_SCC_START)
        assert np.array_equal(res.order[rows], want), "order differs on stream %d" % s
        for name, got in (("release", res.release), ("sent", res.stable_sent)):
            plane = np.full(planes.steps, _lib.FX_RELEASE_NONE, np.uint32)
            for a, step in ref[name].items():
                plane[a] = step
            assert np.array_equal(got[rows], plane), "%s differs on stream %d" % (name, s)
        assert list(res.stable_clock[s]) == ref["stable"], "stable clocks differ on stream %d" % s
    return done


def run(streams, n, thr, keys, refs=None, allow_capacity=False, **kw):
    planes = ft.pack_table_streams(streams, n, keys)
    res = fd.run_table(planes, thr, order_fill=ORDER_TAG, **kw)
    if refs is None:
        refs = [RP.run_stream(st, n, thr, keys, execute_at_commit=kw.get("execute_at_commit", False))
                for st in streams]
    done = compare(planes, res, refs, allow_capacity)
    return planes, res, refs, done


@pytest.mark.parametrize("tier", [None, ONCHIP, HBM])
def test_hand_written_many_copies(tier):
    """The hand-written streams, 11 copies of each in one launch (143 streams:
    more than one 64-stream tile), against the answers written out by hand."""
    names = sorted(TP.HAND) * 11
    streams = [list(TP.HAND[nm][0]) for nm in names]
    planes, res, refs, done = run(streams, TP.HAND_N, TP.HAND_THR, TP.HAND_KEYS, tier=tier)
    assert planes.ps and done == len(names) == 11 * len(TP.HAND) > 64
    for s, nm in enumerate(names):
        _, order, release, sent, err = TP.HAND[nm]
        rows = _lib.index(np.arange(planes.steps), s, planes.steps)
        assert res.err[s] == err and res.nexec[s] == len(order)
        assert [int(x) & 0x7FFFFFFF for x in res.order[rows][:len(order)]] == order
        for plane, want in ((res.release, release), (res.stable_sent, sent)):
            got = {a: int(plane[rows][a]) for a in range(len(streams[s])) if plane[rows][a] != _lib.FX_RELEASE_NONE}
            assert got == want, nm
    if tier is None:
        assert res.status == _lib.FX_ERR_INVALID_ARG and res.reruns == 0  # cases 8 and 9 are errors


def ragged(shards, n, f, conflict):
    """The streams of the generated groups of one configuration, three cut
    short and the longest of a length that is no multiple of 4, with their
    restatement results and the groups' own (uncut)."""
    thr = T.quorum_sizes(n, f, False)[2]
    groups = TP.generated(shards, n, f, conflict)
    streams = [list(st) for sts, _, _ in groups for st in sts]
    refs = [r for _, _, res in groups for r in res]
    for s, cut in ((1, 5), (5, 13), (11, 22)):  # their references are not the shared ones
        streams[s] = streams[s][:len(streams[s]) - cut]
        refs[s] = RP.run_stream(streams[s], n, thr, TP.KEYS)
    longest = max(range(len(streams)), key=lambda s: len(streams[s]))
    if len(streams[longest]) % 4 == 0:
        streams[longest] = streams[longest] + [("S", 0, (1, 1))]
        refs[longest] = RP.run_stream(streams[longest], n, thr, TP.KEYS)
    return thr, groups, streams, refs


@pytest.mark.parametrize("tier", [None, ONCHIP, HBM])
@pytest.mark.parametrize("shards,n,f,conflict", [g + (c,) for g in TP.GROUPS for c in TP.CONFLICTS])
def test_generated_groups(tier, shards, n, f, conflict):
    """8 groups of 2 or 3 shard executors (tests/table_shapes_ps.py; the
    conditions the restatement alone meets are in
    test_table_ps_ref.py::test_generated_groups_cover_the_branches), every
    stream in one launch, ragged lengths, steps not a multiple of 4.  A fixed
    tier may stop a stream with FX_ERR_CAPACITY; ONCHIP must finish exactly the
    streams the restatement says fit, and the driver all of them."""
    thr, groups, streams, refs = ragged(shards, n, f, conflict)
    fits = sum(TP.fits_onchip(r) for r in refs)
    assert fits > len(streams) // 2 and all(TP.fits_hbm(r) for r in refs)
    planes, res, refs, done = run(streams, n, thr, TP.KEYS, refs=refs, allow_capacity=tier is not None, tier=tier)
    assert planes.steps % 4 != 0 and len(set(planes.lengths.tolist())) > 3
    if tier is None:
        assert res.status == 0 and done == planes.S and res.reruns == planes.S - fits
    if tier == ONCHIP:
        assert done == fits
    if tier == HBM:
        assert done == planes.S


@pytest.mark.parametrize("shards,n,f,conflict", [(3, 5, 1, 100), (2, 3, 1, 10)])
def test_closed_loop_on_gpu_output(shards, n, f, conflict):
    """stable_messages over the GPU's stable_sent of each group equals, as a
    multiset, the StableAtShard events of that group's input streams."""
    thr = T.quorum_sizes(n, f, False)[2]
    groups = TP.generated(shards, n, f, conflict)
    streams = [list(st) for sts, _, _ in groups for st in sts]
    planes = ft.pack_table_streams(streams, n, TP.KEYS)
    res = fd.run_table(planes, thr)
    assert res.status == 0 and res.stable_sent is not None
    for i, (sts, commands, _) in enumerate(groups):
        msgs = []
        for g in range(shards):
            msgs += ft.stable_messages(ft.sent_rows(planes, res.stable_sent, i * shards + g), commands, g)
        assert len(msgs) > 20
        assert Counter((t, k, d) for t, k, d, _ in msgs) == Counter(TP.s_events(sts))


def test_escalation_on_buffered_pairs():
    """70 messages for 70 distinct (key, rifl) pairs before their commands are
    stable here: more than FX_TABLE_PS_ONCHIP_BUFFERED, so the stream stops on
    chip and reruns on HBM; a stream with 60 stays on chip."""
    n, thr, keys = 3, 2, 2

    def stream(count):
        st = [("S", i % 2, (1, i + 1)) for i in range(count)]
        return st + [("A", i % 2, (1, i + 1), i // 2 + 1, [(1, i // 2 + 1, i // 2 + 1), (2, i // 2 + 1, i // 2 + 1)], 1, 2)
                     for i in range(count)]

    streams = [stream(70), stream(60)]
    refs = [RP.run_stream(st, n, thr, keys) for st in streams]
    assert [r["max_buffered_pairs"] for r in refs] == [70, 60] and [r["nexec"] for r in refs] == [70, 60]
    assert [TP.fits_onchip(r) for r in refs] == [False, True] and all(TP.fits_hbm(r) for r in refs)
    planes, res, refs, done = run(streams, n, thr, keys, refs=refs)
    assert res.reruns == 1 and res.status == 0 and done == 2
    one = fd.run_table(planes, thr, tier=ONCHIP)
    assert one.err.tolist() == [_lib.FX_ERR_CAPACITY, 0]
    # the HBM tier holds FX_TABLE_PS_HBM_BUFFERED pairs: 520 stop it, 512 (more than one row per lane) do not
    big = [stream(_lib.FX_TABLE_PS_HBM_BUFFERED + 8), stream(_lib.FX_TABLE_PS_HBM_BUFFERED)]
    brefs = [RP.run_stream(st, n, thr, keys) for st in big]
    assert [TP.fits_hbm(r) for r in brefs] == [False, True]
    planes, res, brefs, done = run(big, n, thr, keys, refs=brefs, allow_capacity=True)
    assert res.err.tolist() == [_lib.FX_ERR_CAPACITY, 0] and res.reruns == 2 and done == 1


@pytest.mark.parametrize("tier", [None, HBM])
def test_errors_beside_good_streams(tier):
    X, Y, S1, att, st = TP.X, TP.Y, TP.S1, TP.att, TP.st
    good = list(TP.HAND["followers"][0])
    streams = [
        good,
        list(TP.HAND["count_above_missing"][0]) + good,
        list(TP.HAND["shards_differ"][0]) + good,
        [att(0, X, 1, 1, 2, 2), att(1, X, 1, 1, 3, 2)] + good,               # another nkeys for the dot
        [st(0, X), att(0, X, 1, 1, 1, 2), att(1, S1, 1, 1, 1, 1), ("S", 3, Y)],  # a key beyond the shard's
        [st(0, X), att(0, X, 1, 1, 1, 2), st(1, (4, 1))],                     # a rifl no process issued
        [st(0, X), att(0, X, 1, 1, 1, 2), st(1, (1, 0))],
        # a bad vote range after a message was buffered: the rows of events 0 and 1 stay
        [att(2, S1, 1, 1, 1, 1), st(0, X), ("A", 0, X, 1, [(1, 1, 1), (1, 1, 1)], 1, 2)] + good,
        # the sender of a two-key, two-shard command waits for the other shard: a third event of the dot
        [att(0, X, 1, 1, 2, 2), st(0, X), att(1, X, 1, 1, 2, 2), att(2, X, 1, 1, 2, 2)],
        good,
    ]
    refs = [RP.run_stream(s, TP.HAND_N, TP.HAND_THR, TP.HAND_KEYS) for s in streams]
    packed = [list(s) for s in streams]
    packed[4][3] = ("S", 2, Y)  # (the packer refuses key 3: the header word is set below)
    planes = ft.pack_table_streams(packed, TP.HAND_N, TP.HAND_KEYS)
    planes.hdr[int(_lib.index(3, 4, planes.steps))] = ft.table_hdr_stable(3)
    res = fd.run_table(planes, TP.HAND_THR, order_fill=ORDER_TAG, tier=tier)
    assert compare(planes, res, refs) == len(streams)
    bad, dot = _lib.FX_ERR_INVALID_ARG, _lib.FX_ERR_DOT_RANGE
    assert res.err.tolist() == [0, bad, bad, bad, bad, dot, dot, _lib.FX_ERR_VOTE_RANGE, bad, 0]
    assert res.nexec.tolist() == [3, 1, 1, 0, 2, 1, 1, 1, 1, 3]
    if tier is None:
        assert res.status == bad and res.reruns == 0


@pytest.mark.parametrize("tier", [ONCHIP, HBM])
def test_execute_at_commit(tier):
    """FX_FLAG_EXECUTE_AT_COMMIT with StableAtShard events present: they have no effect."""
    sts, _, _ = TP.generated(3, 5, 1, 10)[0]
    streams = [list(st) for st in sts] + [list(TP.HAND["followers"][0]), list(TP.HAND["count_above_missing"][0])]
    assert all(any(ev[0] == "S" for ev in st) for st in streams)
    planes, res, refs, done = run(streams, 5, 3, TP.KEYS, execute_at_commit=True, tier=tier)
    assert done == 5 and np.all(res.stable_clock == 0) and np.all(res.err == 0)
    assert np.all(res.stable_sent == _lib.FX_RELEASE_NONE)
    assert all(r["nexec"] == sum(ev[0] == "A" for ev in st) for r, st in zip(refs, streams))


@pytest.mark.parametrize("tier", [None, ONCHIP, HBM])
def test_streams_without_the_new_things_equal_the_mk_entry_points(tier):
    """Multi-key streams of one shard through the _ps entry points (nkeys words
    given one shard each) give exactly what the _mk entry points give, and the
    stable_sent plane marks the _mk sender."""
    n, f, tiny = 5, 1, False
    thr = T.quorum_sizes(n, f, tiny)[2]
    streams = [list(st) for st in TM.generated(n, f, tiny, 3, 100)[:12]] + [list(TM.HAND["chain_cut"][0])]
    streams[3] = streams[3][:-7]
    streams.append([TM.att(0, TM.X, 1, 1, 2), TM.att(1, TM.X, 1, 1, 9)])  # FX_ERR_INVALID_ARG
    planes = ft.pack_table_streams(streams, n, TM.KEYS)
    assert planes.nkeys is not None and not planes.ps
    old = fd.run_table(planes, thr, order_fill=ORDER_TAG, tier=tier)
    new = fd.run_table(planes, thr, order_fill=ORDER_TAG, tier=tier, shards=True)
    for field in ("order", "release", "nexec", "err", "stable_clock"):
        assert np.array_equal(getattr(old, field), getattr(new, field)), field
    assert (old.status, old.reruns) == (new.status, new.reruns)
    assert old.stable_sent is None and np.count_nonzero(old.err == _lib.FX_ERR_INVALID_ARG) == 1
    refs = [RP.run_stream(st, n, thr, TM.KEYS) for st in streams]
    assert compare(planes, new, refs, allow_capacity=tier is not None) > len(streams) // 2
    assert sum(len(r["sent"]) for r in refs) > 100
