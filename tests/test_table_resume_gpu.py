"""Resumable table-executor streams (fx_table_advance through
fantoch_amd.device.TableSession) and the closed loop over groups of shard
executors (fantoch_amd.table.run_table_groups) on the GPU.  Whatever the
partition of a stream into calls, every output -- order, release, stable_sent
planes, nexec, err, stable clocks -- must equal, bit for bit, one whole-stream
launch at FX_TABLE_TIER_HBM over the same planes, and the CPU restatement.
GPU only."""
import copy
import random

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import table as ft

import table_edges as E
import table_ref_ps as RP
import table_resume as TR
import table_shapes as T
import table_shapes_mk as TM
import table_shapes_ps as TP

pytestmark = pytest.mark.gpu

SINGLE, MK, PS = TR.SINGLE, TR.MK, TR.PS
HBM = _lib.FX_TABLE_TIER_HBM
TAG, TAG_WORD, NONE = 0xA5, 0xA5A5A5A5, _lib.FX_RELEASE_NONE
BAD = _lib.FX_ERR_INVALID_ARG
PLANES = ("order", "release", "nexec", "err", "stable_clock", "stable_sent")


def session(planes, thr, kind, at_commit=False):
    return fd.TableSession(planes.S, planes.steps, planes.n, planes.keys, planes.vmax, thr, kind, at_commit,
                           order_fill=TAG)


def whole(planes, thr, kind, at_commit=False):
    """The whole streams in one launch at the HBM tier, through the entry point of `kind`."""
    return fd.run_table(planes, thr, execute_at_commit=at_commit, tier=HBM, order_fill=TAG, multi=kind != SINGLE,
                        shards=kind == PS)


def with_lengths(planes, lengths):
    p = copy.copy(planes)
    p.lengths = np.asarray(lengths, np.uint32)
    return p


def equal(got, want):
    """Every output plane, whole: rows nobody wrote hold their fill in both."""
    for name in PLANES:
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), name


def against_ref(planes, res, refs):
    """Every stream against the restatement's dict; unwritten rows at their fill."""
    for s, ref in enumerate(refs):
        rows = _lib.index(np.arange(planes.steps), s, planes.steps)
        assert res.err[s] == ref["err"] and res.nexec[s] == ref["nexec"], s
        want = np.full(planes.steps, TAG_WORD, np.uint32)
        want[:ref["nexec"]] = np.array(ref["order"], np.uint32) | np.uint32(_lib.FX_ORDER_SCC_START)
        assert np.array_equal(res.order[rows], want), "order differs on stream %d" % s
        for name, got in (("release", res.release), ("sent", res.stable_sent)):
            if got is None:
                continue
            plane = np.full(planes.steps, NONE, np.uint32)
            for a, step in ref.get(name, {}).items():
                plane[a] = step
            assert np.array_equal(got[rows], plane), "%s differs on stream %d" % (name, s)
        assert list(res.stable_clock[s]) == ref["stable"], "stable clocks differ on stream %d" % s


def snapshots(stream, cuts, n, thr, keys, at_commit=False):
    """(nexec, err, stable clocks) of the restatement after cuts[i] events."""
    sim = RP.Stream(n, thr, keys, None, at_commit)
    out, fed = [], 0
    for c in cuts:
        for ev in stream[fed:c]:
            sim.feed(ev)
        fed = max(fed, c)
        ref = sim.result()
        out.append((ref["nexec"], ref["err"], ref["stable"]))
    return out


def garbled(planes, lengths):
    """The planes with 0xA5A5A5A5 in every input word but rows [0, lengths[s])."""
    g = with_lengths(planes, lengths)
    names = ["hdr", "dot", "clock"] + (["nkeys"] if planes.nkeys is not None else [])
    keep = np.concatenate([_lib.index(np.arange(int(l)), s, planes.steps) for s, l in enumerate(lengths)])
    for nm in names:
        arr = np.full(planes.plane, TAG_WORD, np.uint32)
        arr[keep] = getattr(planes, nm)[keep]
        setattr(g, nm, arr)
    g.votes = np.full(planes.votes.size, TAG_WORD, np.uint32)
    for p in range(3 * planes.vmax):
        g.votes[p * planes.plane + keep] = planes.votes[p * planes.plane + keep]
    return g


@pytest.mark.parametrize("kind,at_commit", [(SINGLE, False), (MK, False), (PS, False), (PS, True)])
def test_every_cut_of_one_stream(kind, at_commit):
    """L + 1 copies of one generated stream of L rows (more than one
    64-stream tile, every done mod 4): copy s gets its first s rows in call 1,
    with 0xA5A5A5A5 in every row at or above s, and the rest in call 2.
    tests/test_table_resume_cpu.py::test_cut_streams_hold_what_the_cuts_need
    says what the cuts hold: messages left on to_executors, ops in all four
    states, a buffered pair alive."""
    st, thr = TR.cut_stream(kind)
    n, keys, L = TR.CUT_N, TR.CUT_KEYS, len(st)
    planes = ft.pack_table_streams([list(st)] * (L + 1), n, keys)
    assert planes.ps == (kind == PS) and (planes.nkeys is not None) == (kind != SINGLE) and L + 1 > 128
    pre = TR.prefixes(kind, st, n, thr, keys, at_commit)
    sess = session(planes, thr, kind, at_commit)
    one = sess.advance(garbled(planes, np.arange(L + 1)))
    for s in range(L + 1):
        assert (int(one.nexec[s]), int(one.err[s]), list(one.stable_clock[s])) == pre[s], s
    two = sess.advance(planes)
    ref = TR.RUN[kind](list(st), n, thr, keys, execute_at_commit=at_commit)
    against_ref(planes, two, [ref] * (L + 1))
    equal(two, whole(planes, thr, kind, at_commit))
    assert ref["err"] == 0 and ref["nexec"] > 40


@pytest.mark.parametrize("kind", [MK, PS])
def test_hand_cases_cut_at_every_row(kind):
    """The hand-written streams, one copy per cut 0..L: call 1 up to the cut,
    call 2 the rest, call 3 nothing new.  The error cases stop in whichever
    call reaches their failing event and keep their status afterwards."""
    hand = TM.HAND if kind == MK else TP.HAND
    cases = [(nm, c) for nm in sorted(hand) for c in range(len(hand[nm][0]) + 1)]
    streams = [list(hand[nm][0]) for nm, _ in cases]
    planes = ft.pack_table_streams(streams, TP.HAND_N, TP.HAND_KEYS)
    sess = session(planes, TP.HAND_THR, kind)
    one = sess.advance(with_lengths(planes, [c for _, c in cases]))
    for s, (nm, c) in enumerate(cases):
        ref = TR.RUN[kind](streams[s][:c], TP.HAND_N, TP.HAND_THR, TP.HAND_KEYS)
        assert (int(one.nexec[s]), int(one.err[s]), list(one.stable_clock[s])) == \
            (ref["nexec"], ref["err"], ref["stable"]), (nm, c)
    two = sess.advance(planes)
    refs = [TR.RUN[kind](st, TP.HAND_N, TP.HAND_THR, TP.HAND_KEYS) for st in streams]
    against_ref(planes, two, refs)
    equal(two, whole(planes, TP.HAND_THR, kind))
    equal(sess.advance(planes), two)
    if kind == PS:
        assert sum(r["err"] == BAD for r in refs) > 10 and sum(r["err"] == 0 for r in refs) > 20
        for s, (nm, _) in enumerate(cases):  # the answers written out by hand
            _, order, release, sent, err = hand[nm]
            rows = _lib.index(np.arange(planes.steps), s, planes.steps)
            assert two.err[s] == err and [int(x) & 0x7FFFFFFF for x in two.order[rows][:two.nexec[s]]] == order
            assert {a: int(v) for a, v in enumerate(two.stable_sent[rows]) if v != NONE} == sent


def test_one_row_per_call():
    """One _ps stream of about 100 rows, one fx_table_advance per row."""
    fq, _, thr = T.quorum_sizes(3, 1, False)
    st = TP.synth_table_group(7, 2, 3, fq, thr, TP.KEYS, 30, 100, 4, 0, 3, 2, 3)[0][0]
    L = len(st)
    assert 80 <= L <= 130 and len(TR.coverage(st, 3, thr, TP.KEYS)[0]) >= 1
    planes = ft.pack_table_streams([st], 3, TP.KEYS)
    pre = TR.prefixes(PS, st, 3, thr, TP.KEYS)
    sess = session(planes, thr, PS)
    for c in range(1, L + 1):
        res = sess.advance(with_lengths(planes, [c]))
        assert (int(res.nexec[0]), int(res.err[0]), list(res.stable_clock[0])) == pre[c], c
    against_ref(planes, res, [RP.run_stream(st, 3, thr, TP.KEYS)])
    equal(res, whole(planes, thr, PS))


def test_random_partitions():
    """130 generated streams of unequal length (80 shard streams of groups of
    2 and 3, 50 multi-key streams; conflict rates 0 to 100 %) in 4 calls with
    random cut points of their own; every fifth stream has a call with
    nothing new."""
    n, keys = 3, TP.KEYS
    thr = T.quorum_sizes(n, 1, False)[2]
    streams = [list(st) for shards in (2, 3) for c in TP.CONFLICTS for sts, _, _ in TP.generated(shards, n, 1, c)
               for st in sts]
    streams += [list(st) for c in (0, 50, 100) for st in TM.generated(n, 1, False, 3, c)[:17]][:50]
    assert len(streams) == 130 and len({len(st) for st in streams}) > 40
    rng = random.Random(11)
    cuts = []
    for s, st in enumerate(streams):
        c = sorted(rng.randrange(len(st) + 1) for _ in range(3))
        if s % 5 == 0:
            c[1] = c[0]
        cuts.append(c + [len(st)])
    planes = ft.pack_table_streams(streams, n, keys)
    assert planes.ps
    sess = session(planes, thr, PS)
    snaps = [snapshots(st, cuts[s], n, thr, keys) for s, st in enumerate(streams)]
    for call in range(4):
        res = sess.advance(with_lengths(planes, [c[call] for c in cuts]))
        for s in range(len(streams)):
            assert (int(res.nexec[s]), int(res.err[s]), list(res.stable_clock[s])) == snaps[s][call], (call, s)
    against_ref(planes, res, [RP.run_stream(st, n, thr, keys) for st in streams])
    equal(res, whole(planes, thr, PS))
    assert np.all(res.err == 0)


@pytest.mark.parametrize("kind", [SINGLE, MK, PS])
def test_full_registers_carried(kind):
    """512 pending ops -- all eight register rows of every lane, equal clocks
    across rows -- saved directly before the event that releases them all."""
    st = E.mass(512, 3, 3)
    at = 512 + 1  # the second detached range makes clock 7 stable
    planes = ft.pack_table_streams([st, st], 3, 1)
    sess = session(planes, 2, kind)
    one = sess.advance(with_lengths(planes, [at, at - 1]))
    assert one.nexec.tolist() == [0, 0] and one.err.tolist() == [0, 0]
    two = sess.advance(planes)
    assert two.nexec.tolist() == [512, 512]
    against_ref(planes, two, [TR.RUN[kind](st, 3, 2, 1)] * 2)
    equal(two, whole(planes, 2, kind))


@pytest.mark.parametrize("kind", [SINGLE, PS])
def test_ring_windows_carried(kind):
    """Streams whose votes go round the HBM ring, cut at 5 points."""
    streams = [E.gappy(seed, 3, 2, 1500, 2048) for seed in range(2)]
    planes = ft.pack_table_streams(streams, 3, 2)
    sess = session(planes, 2, kind)
    for c in (1, 377, 750, 751, 1202, 1500):
        res = sess.advance(with_lengths(planes, [c, min(1500, c + 2)]))
    refs = [TR.RUN[kind](st, 3, 2, 2) for st in streams]
    assert all(r["max_above"] == 2048 and r["err"] == 0 for r in refs)
    against_ref(planes, res, refs)
    equal(res, whole(planes, 2, kind))


@pytest.mark.parametrize("kind", [MK, PS])
def test_highest_clock_carried(kind):
    """The cut stream lifted so that its highest vote is 2**32 - 1, cut once."""
    st, thr = TR.cut_stream(kind)
    up, pre = E.lift(list(st), (1 << 32) - 1 - E.highest(st), TR.CUT_N, TR.CUT_KEYS)
    assert E.highest(up) == (1 << 32) - 1
    planes = ft.pack_table_streams([up, up], TR.CUT_N, TR.CUT_KEYS)
    sess = session(planes, thr, kind)
    sess.advance(with_lengths(planes, [pre + len(st) // 2, pre - 1]))
    res = sess.advance(planes)
    ref = TR.RUN[kind](up, TR.CUT_N, thr, TR.CUT_KEYS)
    assert ref["err"] == 0 and max(ref["stable"]) == (1 << 32) - 1
    against_ref(planes, res, [ref, ref])
    equal(res, whole(planes, thr, kind))


def test_init_over_garbage_and_again():
    """FX_FLAG_INIT starts from an empty executor whatever `state` holds:
    0xA5 bytes before the first call, a finished session's state before the
    second."""
    st, thr = TR.cut_stream(PS)
    L = len(st)
    planes = ft.pack_table_streams([list(st)] * 3, TR.CUT_N, TR.CUT_KEYS)
    want = whole(planes, thr, PS)
    sess = session(planes, thr, PS)
    sess.state.fill_bytes(0xA5)
    sess.advance(with_lengths(planes, [L // 3, L, 0]))
    equal(sess.advance(planes), want)
    sess.reset()
    sess.advance(with_lengths(planes, [L // 2, 1, L - 1]))
    equal(sess.advance(planes), want)


def test_nothing_new_and_misuse():
    """len == done twice: outputs and state bytes stay.  Another
    stability_threshold, other steps, len < done: FX_ERR_INVALID_ARG for the
    stream with the state bytes as they were; the session then goes on."""
    st, thr = TR.cut_stream(PS)
    L = len(st)
    planes = ft.pack_table_streams([list(st)] * 3, TR.CUT_N, TR.CUT_KEYS)
    sess = session(planes, thr, PS)
    state = lambda: sess.state.download(np.uint8, sess.state_bytes)
    cut = [L // 2, L // 2 + 1, L]
    one = sess.advance(with_lengths(planes, cut))
    before = state()
    for _ in range(2):
        equal(sess.advance(with_lengths(planes, cut)), one)
        assert np.array_equal(state(), before)
    more = with_lengths(planes, [L // 2 + 9, L, L])
    for contract in (dict(stability_threshold=thr + 1), dict(steps=planes.steps + 4)):
        res = sess.advance(more, **contract)
        assert res.err.tolist() == [BAD] * 3 and np.array_equal(res.nexec, one.nexec)
        assert np.array_equal(state(), before)
    res = sess.advance(with_lengths(planes, [L // 2 - 1, L // 2 + 1, L - 4]))
    assert res.err.tolist() == [BAD, 0, BAD] and np.array_equal(res.nexec, one.nexec)
    assert np.array_equal(state(), before)
    equal(sess.advance(planes), whole(planes, thr, PS))


def stop_group():
    """A group whose shard 1 stops with FX_ERR_INVALID_ARG (the hand-written
    count_above_missing) before shard 0's message to it is due."""
    own = [[TP.att(0, TP.S1, 1, 1, 1, 1), ("D", 0, [(3, 1, 1)]), ("D", 2, [(3, 1, 1)]), ("D", 2, [(3, 2, 2)]),
            TP.att(1, TP.Y, 2, 1, 1, 2)], list(TP.HAND["count_above_missing"][0])]
    return own, {TP.Y: {0: [1], 1: [2]}}


@pytest.mark.parametrize("delay", [None, TR.hashed_delay])
@pytest.mark.parametrize("n", [5, 3])
def test_closed_loop(n, delay):
    """run_table_groups over two groups of every configuration with n
    processes (and, with n = 3, one whose second shard stops), one session:
    the streams as handled and every output equal the closed loop on the
    CPU, and each returned stream run whole through fx_table_run_ps gives the
    same rows."""
    thr = T.quorum_sizes(n, 1, False)[2]
    groups = [(TR.own_events(sts), commands) for shards, gn, f in TP.GROUPS if gn == n for c in TP.CONFLICTS
              for sts, commands, _ in TP.generated(shards, gn, f, c, msg_lag=0)[:2]]
    assert len(groups) == 8
    if n == 3:
        groups.append(stop_group())
    out = ft.run_table_groups(groups, n, TP.KEYS, thr, delay=delay)
    streams, results = [], []
    for got, (own, commands) in zip(out, groups):
        sts, refs = TR.closed_loop(own, commands, n, thr, TP.KEYS, delay)
        assert got["streams"] == sts
        for g, (r, w) in enumerate(zip(got["results"], refs)):
            assert all(r[f] == w[f] for f in TR.FIELDS), g
        streams += got["streams"]
        results += got["results"]
    assert sum(r["err"] != 0 for r in results) == (1 if n == 3 else 0)
    assert sum(len(r["sent"]) for r in results) > 100
    planes = ft.pack_table_streams(streams, n, TP.KEYS)
    against_ref(planes, fd.run_table(planes, thr, order_fill=TAG), results)
