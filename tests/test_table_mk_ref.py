"""The multi-key restatement (tests/table_ref_mk.py) on the CPU: it equals the
single-key restatement when every command has one key, gives the orders
written out by hand from executor.rs for the hand-written streams, and over
the generated multi-key streams executes every command on all its keys."""
import pytest

from fantoch_amd import table as ft

import table_ref as R
import table_ref_mk as RM
import table_shapes as T
import table_shapes_mk as TM


@pytest.mark.parametrize("n,f,tiny", T.CONFIGS)
@pytest.mark.parametrize("conflict", T.CONFLICTS)
def test_single_key_streams_equal_the_single_key_restatement(n, f, tiny, conflict):
    thr = T.quorum_sizes(n, f, tiny)[2]
    for st, ref in zip(T.generated(n, f, tiny, conflict), T.generated_ref(n, f, tiny, conflict)):
        got = RM.run_stream(list(st), n, thr, T.KEYS)
        for field in ("order", "release", "nexec", "err", "stable", "max_above"):
            assert got[field] == ref[field], field
        assert got["max_live"] == ref["max_pending"] and got["max_stack"] == got["buffered"] == got["unhandled"] == 0


def test_single_key_kats_and_errors():
    kat = T.KAT["majority"]
    for names in T.majority_streams()[::17]:
        st = T.kat_stream("majority", names)
        ref = R.run_stream(st, kat["n"], kat["stability_threshold"], 1)
        got = RM.run_stream([ev + (1,) for ev in st], kat["n"], kat["stability_threshold"], 1)
        assert (got["order"], got["release"], got["stable"]) == (ref["order"], ref["release"], ref["stable"])
    a1, e2 = T.kat_event("majority", "A1"), T.kat_event("majority", "E2")
    for bad, err in (([a1, e2, e2], R.FX_ERR_DOUBLE_INDEX), ([a1, ("D", 0, [(1, 1, 1)])], R.FX_ERR_VOTE_RANGE),
                     ([a1, ("A", 0, (6, 1), 9, [(4, 1, 1)])], R.FX_ERR_DOT_RANGE), ([("D", 1, [])], R.FX_ERR_INVALID_ARG)):
        ref = R.run_stream(bad, kat["n"], kat["stability_threshold"], 1)
        got = RM.run_stream(bad, kat["n"], kat["stability_threshold"], 1)
        assert got["err"] == ref["err"] == err and got["order"] == ref["order"]


@pytest.mark.parametrize("name", sorted(TM.HAND))
def test_hand_written(name):
    events, order, release, unhandled = TM.HAND[name]
    got = RM.run_stream(events, TM.HAND_N, TM.HAND_THR, TM.HAND_KEYS)
    assert got["err"] == 0
    assert got["order"] == order
    assert got["release"] == release
    assert got["nexec"] == len(order) and got["unhandled"] == unhandled and got["buffered"] == 0


def test_hand_written_details():
    late = RM.run_stream(TM.HAND["late_key"][0], TM.HAND_N, TM.HAND_THR, TM.HAND_KEYS)
    assert late["max_stack"] == 1 and late["max_live"] == 2
    chain = RM.run_stream(TM.HAND["chain"][0], TM.HAND_N, TM.HAND_THR, TM.HAND_KEYS)
    assert chain["release"][1] == chain["release"][2] + 1  # Y's message waited for the next event's drain
    cut = RM.run_stream(TM.HAND["chain_cut"][0], TM.HAND_N, TM.HAND_THR, TM.HAND_KEYS)
    assert 1 not in cut["release"] and cut["unhandled"] == 1
    three = RM.run_stream(TM.HAND["three_keys"][0], TM.HAND_N, TM.HAND_THR, TM.HAND_KEYS)
    assert three["max_stack"] == 2 and three["order"][1:] == [1, 0]  # key 2 before key 0: last pushed first
    # execute_at_commit: every attached event at its own step
    at = RM.run_stream(TM.HAND["chain"][0], TM.HAND_N, TM.HAND_THR, TM.HAND_KEYS, execute_at_commit=True)
    assert at["order"] == [0, 1, 2, 3] and at["release"] == {0: 0, 1: 1, 2: 2, 3: 3} and at["stable"] == [0, 0, 0]


def test_input_contract():
    run = lambda ev: RM.run_stream(ev, TM.HAND_N, TM.HAND_THR, TM.HAND_KEYS)
    X = TM.X
    assert run([TM.att(0, X, 1, 1, 2), TM.att(1, X, 1, 1, 3)])["err"] == R.FX_ERR_INVALID_ARG  # another nkeys
    assert run([TM.att(0, X, 1, 1, 2), TM.att(1, X, 2, 1, 2)])["err"] == R.FX_ERR_INVALID_ARG  # another clock
    # the same key again: the op has left the votes table and waits in the queue
    assert run([TM.att(0, X, 1, 1, 2), TM.att(0, X, 1, 2, 2)])["err"] == R.FX_ERR_INVALID_ARG
    # ... still in the votes table: the reference's own panic (mod.rs:163-165)
    assert run([("A", 0, X, 1, [(1, 1, 1)], 2), ("A", 0, X, 1, [(2, 1, 1)], 2)])["err"] == R.FX_ERR_DOUBLE_INDEX
    assert run([TM.att(0, X, 1, 1, 9)])["err"] == R.FX_ERR_INVALID_ARG and run([TM.att(0, X, 1, 1, 0)])["err"] == 1
    # a third event of a two-key command whose first partial still waits for its message
    third = run([TM.att(0, TM.Y, 1, 1, 2), TM.att(2, X, 2, 1, 2), TM.att(0, X, 2, 2, 2), TM.att(1, TM.Y, 1, 1, 2),
                 TM.att(1, X, 2, 2, 2)])
    assert third["err"] == R.FX_ERR_INVALID_ARG and third["order"] == [3, 0, 2]
    # a vote-range error in the middle of a command: earlier rows stay
    mid = run([TM.att(0, X, 1, 1, 2), TM.att(2, TM.S1, 1, 1, 1), ("A", 1, X, 1, [(1, 1, 1), (1, 1, 1)], 2)])
    assert mid["err"] == R.FX_ERR_VOTE_RANGE and mid["order"] == [1] and mid["release"] == {1: 1}


@pytest.mark.parametrize("n,f,tiny", TM.CONFIGS)
@pytest.mark.parametrize("kmax", TM.KMAX)
@pytest.mark.parametrize("conflict", TM.CONFLICTS)
def test_generated_streams_execute_every_command_on_all_keys(n, f, tiny, kmax, conflict):
    streams = TM.generated(n, f, tiny, kmax, conflict)
    refs = TM.generated_ref(n, f, tiny, kmax, conflict)
    seen = set()
    for st, ref in zip(streams, refs):
        attached = [r for r, ev in enumerate(st) if ev[0] == "A"]
        assert ref["err"] == 0 and ref["unhandled"] == 0
        assert sorted(ref["order"]) == attached and sorted(ref["release"]) == attached
        assert ref["buffered"] == 0  # a StableAtShard never arrives early at one shard
        assert all(ref["release"][a] >= a for a in attached)
        # per key the partials execute in (clock, dot) order (the reference's per-key monitor)
        for key in range(TM.KEYS):
            ids = [(st[a][3], st[a][2]) for a in ref["order"] if st[a][1] == key]
            assert ids == sorted(ids)
        seen.update(ev[5] for ev in st if ev[0] == "A")
        # Tempo's shape: the events of a command are adjacent, keys ascending and distinct
        i = 0
        while i < len(st):
            if st[i][0] == "A":
                k = st[i][5]
                grp = st[i:i + k]
                assert all(e[0] == "A" and e[2] == st[i][2] and e[3] == st[i][3] and e[5] == k for e in grp)
                assert [e[1] for e in grp] == sorted({e[1] for e in grp})
                i += k
            else:
                i += 1
    assert seen == set(range(1, kmax + 1))


def test_pack_roundtrip_and_nkeys_plane():
    streams = [list(TM.HAND["chain"][0]), [T.kat_event("majority", "A1")]]
    planes = ft.pack_table_streams(streams, 5, 3)
    assert planes.nkeys is not None and planes.stream(0) == streams[0] and planes.stream(1) == streams[1]
    assert ft.pack_table_streams([streams[1], [streams[1][0] + (1,)]], 5, 3).nkeys is None
    with pytest.raises(ValueError):
        ft.pack_table_streams([[("A", 0, (1, 1), 1, [], 2, 3)]], 5, 1)
