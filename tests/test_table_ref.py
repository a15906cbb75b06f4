"""The CPU restatement of Tempo's TableExecutor (tests/table_ref.py) against
the reference's own tests (tests/golden/table_kat.json), the packer's round
trip, the validity of the generated streams, Tempo's quorum sizes and the
argument checks of fx_table_execute.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import table as ft

import table_ref as R
import table_shapes as T


def names_of(case, stream_names, arrivals):
    return [stream_names[a] for a in arrivals]


def test_majority_kat_stepwise_and_all_permutations():
    kat = T.KAT["majority"]
    res = R.run_stream(T.kat_stream("majority", kat["stepwise"]), kat["n"], kat["stability_threshold"], 1)
    assert res["err"] == 0
    assert [names_of("majority", kat["stepwise"], st) for st in res["steps"]] == kat["stepwise_stable"]
    assert [res["release"][a] for a in res["order"]] == [0, 2, 2, 4, 4]
    streams = T.majority_streams()
    assert len(streams) == 121
    for names in streams:
        res = R.run_stream(T.kat_stream("majority", names), kat["n"], kat["stability_threshold"], 1)
        assert res["err"] == 0 and names_of("majority", names, res["order"]) == kat["total_order"]


def test_tiny_quorums_kat():
    kat = T.KAT["tiny"]
    res = R.run_stream(T.kat_stream("tiny", kat["stepwise"]), kat["n"], kat["stability_threshold"], 1)
    assert res["err"] == 0
    assert [names_of("tiny", kat["stepwise"], st) for st in res["steps"]] == kat["stepwise_stable"]


def test_detached_votes_kat():
    kat = T.KAT["detached"]
    events = T.detached_events()
    for i, expect in enumerate(kat["stable_after"]):
        res = R.run_stream(events[:i + 1], kat["n"], kat["stability_threshold"], 2)
        assert res["err"] == 0 and res["nexec"] == 0 and res["stable"] == expect


def test_restatement_errors():
    a1 = T.kat_event("majority", "A1")
    good = T.kat_stream("majority", T.KAT["majority"]["stepwise"])
    # the same (clock, dot) while the first is pending (mod.rs:163-165); E2 stays pending alone
    e2 = T.kat_event("majority", "E2")
    assert R.run_stream([e2, e2], 5, 3, 1)["err"] == R.FX_ERR_DOUBLE_INDEX
    for bad in ([(1, 1, 1)], [(6, 1, 1)], [(2, 0, 1)], [(2, 3, 2)]):  # repeated, voter n + 1, start 0, start > end
        res = R.run_stream([a1, ("D", 0, bad)] + good, 5, 3, 1)
        assert res["err"] == R.FX_ERR_VOTE_RANGE and res["nexec"] == 1 and res["stable"] == [1]
    assert R.run_stream([("A", 0, (6, 1), 1, [])], 5, 3, 1)["err"] == R.FX_ERR_DOT_RANGE
    res = R.run_stream(good, 5, 3, 1, execute_at_commit=True)
    assert res["order"] == [0, 1, 2, 3, 4] and res["stable"] == [0]


def test_packer_round_trip_and_limits():
    streams = [list(st) for st in T.generated(5, 2, False, 10)[:5]] + [T.detached_events(), []]
    planes = ft.pack_table_streams(streams, 5, T.KEYS)
    assert planes.S == len(streams) and planes.vmax == 4 and list(planes.lengths) == [len(s) for s in streams]
    for s, st in enumerate(streams):
        assert planes.stream(s) == st
    h = int(planes.hdr[int(_lib.index(0, 0, planes.steps))])
    ev = streams[0][0]
    assert h == ft.table_hdr(0 if ev[0] == "A" else 1, len(ev[-1]), ev[1])
    with pytest.raises(ValueError):
        ft.pack_table_streams([[("A", 0, (1, 1), 1 << 32, [])]], 5, 1)
    with pytest.raises(ValueError):
        ft.pack_table_streams([[("D", 0, [(1, 1, 1 << 32)])]], 5, 1)
    with pytest.raises(ValueError):
        ft.pack_table_streams([[("D", 3, [(1, 1, 1)])]], 5, 3)


@pytest.mark.parametrize("conflict", T.CONFLICTS)
@pytest.mark.parametrize("n,f,tiny", T.CONFIGS)
def test_generated_streams_are_valid(n, f, tiny, conflict):
    """No reference assertion fails, and every attached command executes
    exactly once by the end of the stream."""
    streams, refs = T.generated(n, f, tiny, conflict), T.generated_ref(n, f, tiny, conflict)
    assert len(streams) == T.SEEDS
    for st, res in zip(streams, refs):
        attached = [i for i, ev in enumerate(st) if ev[0] == "A"]
        assert len(attached) == T.CMDS
        assert res["err"] == 0
        assert sorted(res["order"]) == attached
    assert streams == T.generated.__wrapped__(n, f, tiny, conflict)  # deterministic


def test_tempo_quorum_sizes(lib):
    for row in T.KAT["tempo_parameters"]:
        assert list(ft.tempo_quorum_sizes(row["n"], row["f"], row["tiny"])) == row["sizes"]
        assert list(T.quorum_sizes(row["n"], row["f"], row["tiny"])) == row["sizes"]
    q = ctypes.c_uint32()
    assert lib.fx_tempo_quorum_sizes(0, 0, 0, ctypes.byref(q), ctypes.byref(q), ctypes.byref(q)) == \
        _lib.FX_ERR_INVALID_ARG
    assert lib.fx_tempo_quorum_sizes(5, 1, 0, None, ctypes.byref(q), ctypes.byref(q)) == _lib.FX_ERR_INVALID_ARG


def test_status_string(lib):
    assert b"vote" in lib.fx_status_string(_lib.FX_ERR_VOTE_RANGE)


def test_bad_args_rejected_without_a_device(lib):
    """Argument errors come before any device call (host pointers stand in
    for planes: nothing dereferences them)."""
    w = np.zeros(256, np.uint32)
    p = w.ctypes.data
    out = _lib.OrderBatch(p, p, p, p)

    def call(n=5, thr=3, vmax=3, keys=4, hdr=p, votes=p, outb=out, tier=0, flags=0):
        inb = _lib.TableBatch(hdr, p, p, votes, None, 1, 4, n, keys, vmax, thr)
        return lib.fx_table_execute(ctypes.byref(inb), ctypes.byref(outb) if outb else None, None, None, 1, tier,
                                    None, flags, None)

    bad = _lib.FX_ERR_INVALID_ARG
    assert call(n=0) == bad and call(n=17) == bad
    assert call(thr=6) == bad and call(thr=0) == bad
    assert call(vmax=0) == bad and call(vmax=65) == bad
    assert call(keys=0) == bad
    assert call(hdr=None) == bad and call(votes=None) == bad and call(outb=None) == bad
    assert call(outb=_lib.OrderBatch(p, None, p, p)) == bad
    assert call(tier=2) == bad and call(tier=1) == bad  # the HBM tier needs its state
    assert call(flags=_lib.FX_FLAG_SAVE_STATE) == bad
    assert lib.fx_table_execute(None, None, None, None, 0, 0, None, 0, None) == bad
    assert lib.fx_table_run(None, None, None, 0, None, None) == bad
    if lib.fx_device_count() <= 0:
        assert call() == _lib.FX_ERR_NO_DEVICE
        inb = _lib.TableBatch(p, p, p, p, None, 1, 4, 5, 64, 3, 3)  # keys beyond the on-chip tier
        assert lib.fx_table_run(ctypes.byref(inb), ctypes.byref(out), None, 0, None, None) == _lib.FX_ERR_NO_DEVICE
    assert lib.fx_table_state_bytes(5, 8, 3) == 8 * 16 * (1 + _lib.FX_TABLE_HBM_WINDOW // 32) * 4 * 3
