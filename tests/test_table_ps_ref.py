"""The restatement of the table executor over several shards
(tests/table_ref_ps.py) on the CPU: the hand-written streams against the
answers written out by hand from executor.rs, single-shard streams against
tests/table_ref_mk.py, the packing of the new event and word, and the
conditions on the generated groups that make the GPU test mean something."""
from collections import Counter

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import table as ft

import table_ref_mk as RM
import table_ref_ps as RP
import table_shapes_mk as TM
import table_shapes_ps as TP


@pytest.mark.parametrize("name", sorted(TP.HAND))
def test_hand_written(name):
    events, order, release, sent, err = TP.HAND[name]
    got = RP.run_stream(events, TP.HAND_N, TP.HAND_THR, TP.HAND_KEYS)
    assert got["err"] == err
    assert got["order"] == order and got["nexec"] == len(order)
    assert got["release"] == release
    assert got["sent"] == sent


def test_hand_written_details():
    run = lambda name, **kw: RP.run_stream(TP.HAND[name][0], TP.HAND_N, TP.HAND_THR, TP.HAND_KEYS, **kw)
    assert run("three_both_buffered")["max_count"] == 2 and run("three_both_buffered")["max_buffered_pairs"] == 1
    assert run("three_one_each")["max_count"] == 1 and run("three_one_each")["buffered"] == 1
    first = run("two_keys_msgs_first")
    assert first["max_buffered_pairs"] == 2 and first["max_stack"] == 1  # the local message went through the drain
    assert run("two_keys_msgs_last")["buffered"] == 0
    assert run("msg_for_queued")["buffered"] == 1 and run("wait_then_msg")["buffered"] == 0
    nobody = run("msg_for_nobody")
    assert nobody["buffered"] == 1 and nobody["err"] == 0
    # the stream of case 8 stops before the failing try is recorded; a prefix without that event is fine
    assert RP.run_stream(TP.HAND["count_above_missing"][0][:3], TP.HAND_N, TP.HAND_THR, TP.HAND_KEYS)["err"] == 0
    # execute_at_commit: every attached event at its own step, StableAtShard events without effect
    eac = run("followers", execute_at_commit=True)
    assert eac["order"] == [0, 1, 2, 3, 4] and eac["sent"] == {} and eac["buffered"] == 0
    # a StableAtShard event is checked like any other: key, then the dot
    bad = lambda ev: RP.run_stream([ev], TP.HAND_N, TP.HAND_THR, TP.HAND_KEYS)["err"]
    assert bad(("S", 3, TP.X)) == _lib.FX_ERR_INVALID_ARG
    assert bad(("S", 0, (4, 1))) == bad(("S", 0, (1, 0))) == _lib.FX_ERR_DOT_RANGE


@pytest.mark.parametrize("n,f,tiny", TM.CONFIGS)
@pytest.mark.parametrize("kmax,conflict", [(2, 10), (3, 100)])
def test_single_shard_streams_equal_the_multi_key_restatement(n, f, tiny, kmax, conflict):
    thr = TP.quorum_sizes(n, f, tiny)[2]
    for st, ref in zip(TM.generated(n, f, tiny, kmax, conflict), TM.generated_ref(n, f, tiny, kmax, conflict)):
        got = RP.run_stream(list(st), n, thr, TM.KEYS)
        assert {k: got[k] for k in ref} == ref
        assert got["max_buffered_pairs"] == got["max_count"] == 0
        # stable_sent marks the _mk sender: one row per command with more than one key
        assert len(got["sent"]) == len({ev[2] for ev in st if ev[0] == "A" and ev[5] > 1})
    for name, (events, order, release, unhandled) in TM.HAND.items():
        got = RP.run_stream(events, TM.HAND_N, TM.HAND_THR, TM.HAND_KEYS)
        assert (got["order"], got["release"], got["unhandled"], got["err"]) == (order, release, unhandled, 0), name
        assert got == dict(RM.run_stream(events, TM.HAND_N, TM.HAND_THR, TM.HAND_KEYS), sent=got["sent"],
                           max_buffered_pairs=0, max_count=0)


def test_packing():
    """Streams without the new things pack as before; with them the nkeys
    plane holds FX_TABLE_PS_WORD and the planes decode back."""
    old = [list(st) for st in TM.generated(3, 1, False, 2, 10)[:3]]
    p = ft.pack_table_streams(old, 3, TM.KEYS)
    q = ft.pack_table_streams([[ev + (1,) if ev[0] == "A" else ev for ev in st] for st in old], 3, TM.KEYS)
    assert not p.ps and not q.ps and p.nkeys is not None and max(p.nkeys) <= TM.KMAX[-1]
    for name in ("hdr", "dot", "clock", "votes", "nkeys", "lengths"):
        assert np.array_equal(getattr(p, name), getattr(q, name)), name
    single = ft.pack_table_streams([[("A", 0, (1, 1), 1, [(1, 1, 1)])]], 3, 2)
    assert single.nkeys is None and not single.ps
    streams = [list(TP.HAND[name][0]) for name in sorted(TP.HAND)]
    ps = ft.pack_table_streams(streams, TP.HAND_N, TP.HAND_KEYS)
    assert ps.ps and ps.nkeys is not None
    assert [ps.stream(s) for s in range(ps.S)] == [
        [ev[:5] if ev[0] == "A" and ev[5:] == (1, 1) else ev for ev in st] for st in streams]
    at = int(_lib.index(1, sorted(TP.HAND).index("three_one_each"), ps.steps))
    assert ps.nkeys[at] == ft.table_ps_word(1, 3) == 0x301
    at = int(_lib.index(0, sorted(TP.HAND).index("msg_for_nobody"), ps.steps))
    assert ps.nkeys[at] == 0x101  # one key, one shard in a ps plane
    at = int(_lib.index(1, sorted(TP.HAND).index("msg_for_nobody"), ps.steps))
    assert ps.hdr[at] == ft.table_hdr_stable(1) == (1 << 31) | (127 << 24) | 1 and ps.dot[at] == _lib.pack_dot(*TP.X)
    only_s = ft.pack_table_streams([[("S", 0, (1, 1))]], 3, 1)
    assert only_s.ps and only_s.nkeys is None and only_s.vmax == 1
    with pytest.raises(ValueError):
        ft.pack_table_streams([[("S", 0, (1, 1), 1)]], 3, 1)
    with pytest.raises(ValueError):
        ft.pack_table_streams([[("S", 1, (1, 1))]], 3, 1)
    with pytest.raises(ValueError):
        ft.pack_table_streams([[("A", 0, (1, 1), 1, [], 256, 2)]], 3, 1)


def test_stable_messages():
    commands = {(1, 1): {0: [3], 1: [0, 2], 2: [5, 1]}, (2, 1): {1: [4]}, (3, 1): {1: [1], 2: [0]}}
    sent = [((3, 1), 2), ((1, 1), 7), ((2, 1), 7)]
    assert ft.stable_messages(sent, commands, 1) == [(2, 0, (3, 1), 2), (0, 3, (1, 1), 7), (2, 1, (1, 1), 7),
                                                    (2, 5, (1, 1), 7)]
    assert ft.stable_messages([], commands, 0) == []


def group_messages(streams, commands, sents):
    """The messages stable_messages derives from every shard's (row -> step) map."""
    out = []
    for g, sent in enumerate(sents):
        pairs = [(streams[g][a][2], step) for step, a in sorted((step, a) for a, step in sent.items())]
        out += ft.stable_messages(pairs, commands, g)
    return out


def test_generated_groups_cover_the_branches():
    """The groups the GPU test runs (tests/table_shapes_ps.py: G = 2 and 3
    shards, n = 5 and 3 with f = 1, 1..2 keys per shard, about 60 commands per
    shard executor, 16 keys per shard, 10 and 100 % conflicts, 8 seeds each),
    on the restatement alone, so the GPU test cannot pass by leaving cases out.

    lag 4, window 0 and msg_lag 3 were chosen here.  Observed, per
    configuration (G, n, conflict %): streams that buffer a message / reach a
    buffered count of 2 / fit the ONCHIP tier, of streams:
      (2, 5, 10) 16 / 0 / 16 of 16    (2, 5, 100) 14 / 0 / 13 of 16
      (3, 5, 10) 24 / yes / 24 of 24  (3, 5, 100) 24 / yes / 14 of 24
      (2, 3, 10) 16 / 0 / 16 of 16    (2, 3, 100) 15 / 0 / 12 of 16
      (3, 3, 10) 24 / yes / 24 of 24  (3, 3, 100) 24 / yes / 18 of 24
    At most 12 pairs are buffered at once and 23 ops live; what stops a stream
    on chip is a vote more than FX_TABLE_ONCHIP_WINDOW above its voter's
    frontier (up to 76) at 100 % conflicts.  With a window of 1 or 2 (commits
    delivered late) at most half of the 100 % streams of three shards at n = 5
    fit (3 to 12 of 24); with window 0 and lag 0..1 all do.  Every command
    executes on every key, and the streams hold about 900 to 3,000
    StableAtShard events per configuration."""
    for shards, n, f in TP.GROUPS:
        for conflict in TP.CONFLICTS:
            groups = TP.generated(shards, n, f, conflict)
            refs = [r for _, _, res in groups for r in res]
            assert len(refs) == shards * TP.SEEDS
            assert all(r["err"] == 0 for r in refs)
            assert sum(r["buffered"] > 0 for r in refs) * 4 >= len(refs)
            if shards == 3:
                assert max(r["max_count"] for r in refs) == 2
            assert sum(TP.fits_onchip(r) for r in refs) * 2 > len(refs)
            assert all(TP.fits_hbm(r) for r in refs)
            for streams, commands, res in groups:
                # every shard's restatement, run over the finished stream, is the co-simulation's
                thr = TP.quorum_sizes(n, f, False)[2]
                assert [RP.run_stream(st, n, thr, TP.KEYS) for st in streams] == list(res)
                assert all(r["nexec"] == sum(ev[0] == "A" for ev in st) for r, st in zip(res, streams))
                msgs = group_messages(streams, commands, [r["sent"] for r in res])
                assert Counter((t, k, d) for t, k, d, _ in msgs) == Counter(TP.s_events(streams))
                assert len(msgs) > 20
    assert any(not TP.fits_onchip(r) for cfg in TP.GROUPS for _, _, res in TP.generated(*cfg, 100) for r in res)
