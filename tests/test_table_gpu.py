"""GPU table executor (fx_table_run / fx_table_execute) against the CPU
restatement (tests/table_ref.py), bit for bit: order plane, release plane,
nexec, status and the stable clocks.  GPU only."""
import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import table as ft

import table_ref as R
import table_shapes as T

pytestmark = pytest.mark.gpu

ORDER_TAG = 0xA5
ORDER_TAG_WORD = 0xA5A5A5A5


def compare(planes, res, refs, allow_capacity=False):
    """Every stream against its restatement; with allow_capacity a stream may
    instead have stopped with FX_ERR_CAPACITY.  Returns the streams compared.
    Rows beyond nexec (order) and rows of detached events, of commands not
    executed and beyond the stream's length (release) must be untouched."""
    done = 0
    for s, ref in enumerate(refs):
        L = int(planes.lengths[s])
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
        assert L <= planes.steps and list(res.stable_clock[s]) == ref["stable"], "stable clocks differ on stream %d" % s
    return done


def run(streams, n, thr, keys, refs=None, allow_capacity=False, **kw):
    planes = ft.pack_table_streams(streams, n, keys)
    res = fd.run_table(planes, thr, order_fill=ORDER_TAG, **kw)
    if refs is None:
        refs = [R.run_stream(st, n, thr, keys, execute_at_commit=kw.get("execute_at_commit", False))
                for st in streams]
    done = compare(planes, res, refs, allow_capacity)
    return planes, res, refs, done


def test_majority_kat_121_streams():
    kat = T.KAT["majority"]
    names = T.majority_streams()
    planes, res, refs, _ = run([T.kat_stream("majority", nm) for nm in names], kat["n"], kat["stability_threshold"], 1)
    assert planes.S == 121 and res.status == 0 and res.reruns == 0
    for s, nm in enumerate(names):
        rows = _lib.index(np.arange(5), s, planes.steps)
        assert [nm[int(x) & 0x7FFFFFFF] for x in res.order[rows]] == kat["total_order"]
    rows = _lib.index(np.arange(5), 120, planes.steps)
    step = [int(x) & 0x7FFFFFFF for x in res.order[rows]]
    assert [int(res.release[int(_lib.index(a, 120, planes.steps))]) for a in step] == [0, 2, 2, 4, 4]


def test_tiny_quorums_kat():
    kat = T.KAT["tiny"]
    planes, res, refs, _ = run([T.kat_stream("tiny", kat["stepwise"])], kat["n"], kat["stability_threshold"], 1)
    rows = _lib.index(np.arange(5), 0, planes.steps)
    got = [(kat["stepwise"][int(x) & 0x7FFFFFFF], int(res.release[int(_lib.index(int(x) & 0x7FFFFFFF, 0, planes.steps))]))
           for x in res.order[rows]]
    assert got == [("A1", 2), ("E1", 2), ("C1", 4), ("A2", 4), ("D1", 4)]


def test_detached_votes_prefixes():
    kat = T.KAT["detached"]
    events = T.detached_events()
    planes = ft.pack_table_streams([events] * 6, kat["n"], 2)
    planes.lengths = np.arange(1, 7, dtype=np.uint32)  # stream i = the first i + 1 events
    res = fd.run_table(planes, kat["stability_threshold"], order_fill=ORDER_TAG)
    assert np.all(res.err == 0) and np.all(res.nexec == 0)
    assert res.stable_clock.tolist() == kat["stable_after"]
    assert np.all(res.order == ORDER_TAG_WORD) and np.all(res.release == _lib.FX_RELEASE_NONE)


@pytest.mark.parametrize("tier", [None, _lib.FX_TABLE_TIER_ONCHIP, _lib.FX_TABLE_TIER_HBM])
@pytest.mark.parametrize("n,f,tiny,conflict", [cfg + (c,) for cfg in T.CONFIGS for c in T.CONFLICTS])
def test_generated_streams(tier, n, f, tiny, conflict):
    """24 streams, ragged lengths, steps not a multiple of 4 (a stream that
    was cut short keeps commands pending); a fixed tier may stop a stream with
    FX_ERR_CAPACITY, and at lag = 6 the on-chip tier must finish most."""
    thr = T.quorum_sizes(n, f, tiny)[2]
    streams = [list(st) for st in T.generated(n, f, tiny, conflict)]
    refs = list(T.generated_ref(n, f, tiny, conflict))
    for s, cut in ((1, 5), (5, 13), (11, 22)):  # cut three short: their references are not the shared ones
        streams[s] = streams[s][:len(streams[s]) - cut]
        refs[s] = R.run_stream(streams[s], n, thr, T.KEYS)
    longest = max(range(len(streams)), key=lambda s: len(streams[s]))
    if len(streams[longest]) % 4 == 0:
        streams[longest] = streams[longest] + [("D", 0, [])]  # an event without votes
        refs[longest] = R.run_stream(streams[longest], n, thr, T.KEYS)
    planes, res, refs, done = run(streams, n, thr, T.KEYS, refs=refs, allow_capacity=tier is not None, tier=tier)
    assert planes.steps % 4 != 0 and len(set(planes.lengths.tolist())) > 3
    if tier is None:
        assert res.status == 0
    if tier == _lib.FX_TABLE_TIER_ONCHIP:
        assert done > planes.S // 2
    if tier == _lib.FX_TABLE_TIER_HBM:
        assert done == planes.S


def test_generated_70_streams_ragged_tile():
    n, f, tiny = 5, 1, False
    thr = T.quorum_sizes(n, f, tiny)[2]
    streams = [list(st) for st in T.generated(n, f, tiny, 10, count=70)]
    streams[69] = streams[69][:-3]
    planes, res, refs, done = run(streams, n, thr, T.KEYS)
    assert planes.S == 70 and planes.S % 64 != 0 and done == 70 and res.status == 0


def test_escalation():
    """A long lag at 100 % conflicts: the restatement says the stream needs
    more than the on-chip tier holds, so it stops there and reruns on HBM."""
    n, f, tiny = 5, 1, False
    fq, _, thr = T.quorum_sizes(n, f, tiny)
    streams = [ft.synth_table_streams(seed, n, fq, T.KEYS, 150, 100, 80, 4) for seed in range(3)]
    streams += [list(st) for st in T.generated(n, f, tiny, 10)[:3]]
    refs = [R.run_stream(st, n, thr, T.KEYS) for st in streams]
    over = [r["max_pending"] > _lib.FX_TABLE_ONCHIP_PENDING or r["max_above"] > _lib.FX_TABLE_ONCHIP_WINDOW
            for r in refs]
    assert over == [True] * 3 + [False] * 3
    assert all(r["max_pending"] <= _lib.FX_TABLE_HBM_PENDING and r["max_above"] <= _lib.FX_TABLE_HBM_WINDOW
               for r in refs)
    planes, res, refs, done = run(streams, n, thr, T.KEYS, refs=refs)
    assert res.reruns == 3 and res.status == 0 and done == 6
    one = fd.run_table(planes, thr, tier=_lib.FX_TABLE_TIER_ONCHIP)
    assert one.err.tolist() == [_lib.FX_ERR_CAPACITY] * 3 + [0] * 3


def test_many_votes_and_keys_beyond_the_onchip_tier():
    """More than four vote ranges per event (the slots beyond the prefetched
    row), and a key count the on-chip tier does not take: fx_table_run starts
    at HBM, a fixed on-chip launch reports FX_ERR_UNSUPPORTED."""
    n, f, tiny = 7, 3, False
    fq, _, thr = T.quorum_sizes(n, f, tiny)
    streams = [ft.synth_table_streams(seed, n, fq, 40, 30, 10, 6, 4) for seed in range(4)]
    planes, res, refs, done = run(streams, n, thr, 40)
    assert planes.vmax == 6 and res.reruns == 0 and done == 4 and res.status == 0
    with pytest.raises(_lib.FxError) as e:
        fd.run_table(planes, thr, tier=_lib.FX_TABLE_TIER_ONCHIP)
    assert e.value.status == _lib.FX_ERR_UNSUPPORTED


@pytest.mark.parametrize("tier", [_lib.FX_TABLE_TIER_ONCHIP, _lib.FX_TABLE_TIER_HBM])
def test_execute_at_commit(tier):
    streams = [list(st) for st in T.generated(5, 2, False, 10)[:5]]
    planes, res, refs, done = run(streams, 5, 3, T.KEYS, execute_at_commit=True, tier=tier)
    assert done == 5 and np.all(res.stable_clock == 0)
    assert all(r["nexec"] == T.CMDS for r in refs)


@pytest.mark.parametrize("tier", [None, _lib.FX_TABLE_TIER_HBM])
def test_errors_beside_a_good_stream(tier):
    kat = T.KAT["majority"]
    good = T.kat_stream("majority", kat["stepwise"])
    a1, e2 = T.kat_event("majority", "A1"), T.kat_event("majority", "E2")
    streams = [good, [a1, e2, e2] + good]
    # repeated range, voter n + 1, start 0, start > end; then a bad range second in its event
    for bad in ([(1, 1, 1)], [(6, 1, 1)], [(2, 0, 1)], [(2, 3, 2)], [(4, 1, 1), (4, 1, 1)]):
        streams.append([a1, ("D", 0, bad)] + good)
    streams.append([a1, ("A", 0, (6, 1), 9, [(4, 1, 1)])] + good)
    streams.append(good)
    planes, res, refs, done = run(streams, kat["n"], kat["stability_threshold"], 1, tier=tier)
    assert done == len(streams)
    assert res.err.tolist() == [0, _lib.FX_ERR_DOUBLE_INDEX] + [_lib.FX_ERR_VOTE_RANGE] * 5 + \
        [_lib.FX_ERR_DOT_RANGE, 0]
    assert res.nexec.tolist() == [5, 1, 1, 1, 1, 1, 1, 1, 5]
    if tier is None:
        assert res.status == _lib.FX_ERR_DOUBLE_INDEX and res.reruns == 0


def test_profile_slot():
    import ctypes
    lib = _lib.load()
    lib.fx_profile_enable(1)
    try:
        run([T.kat_stream("majority", T.KAT["majority"]["stepwise"])], 5, 3, 1, tier=_lib.FX_TABLE_TIER_ONCHIP)
        ms = ctypes.c_float(-1)
        assert lib.fx_profile_slot_ms(_lib.FX_PROFILE_SLOT_TABLE + _lib.FX_TABLE_TIER_ONCHIP, ctypes.byref(ms)) == 0
        assert ms.value >= 0
    finally:
        lib.fx_profile_enable(0)
