"""fx_table_advance and fantoch_amd.table.run_table_groups without a GPU: the
C ABI (symbols, constants, sizes, argument checks), the routing logic of the
closed loop over a restatement-backed session, and what the restatement says
of the streams the GPU cut tests use.  CPU only."""
import ctypes
import os
import re

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import table as ft

import table_resume as TR
import table_shapes as T
import table_shapes_ps as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [TR.SINGLE, TR.MK, TR.PS]


# ------------------------------------------------------------------ C ABI
def test_symbols_and_constants(lib):
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for name in ("fx_table_session_bytes", "fx_table_advance"):
        assert hasattr(lib, name) and name in bound
    text = open(os.path.join(ROOT, "include", "fantoch_amd.h")).read()
    for name in ("FX_TABLE_KIND_SINGLE", "FX_TABLE_KIND_MK", "FX_TABLE_KIND_PS"):
        assert int(re.search(r"#define %s (\d+)u" % name, text).group(1)) == getattr(_lib, name)
    assert int(re.search(r"#define FX_PROFILE_SLOTS (\d+)u", text).group(1)) > _lib.FX_PROFILE_SLOT_TABLE + 2


@pytest.mark.parametrize("kind", KINDS)
def test_session_bytes(lib, kind):
    tables = lib.fx_table_state_bytes_ps if kind == TR.PS else lib.fx_table_state_bytes
    for keys in (1, 16, 999):
        one = lib.fx_table_session_bytes(kind, 5, keys, 1)
        assert one >= tables(5, keys, 1) and one % 4 == 0
        assert [lib.fx_table_session_bytes(kind, 5, keys, s) for s in (0, 2, 130)] == [0, 2 * one, 130 * one]
    assert lib.fx_table_session_bytes(3, 5, 16, 1) == 0


def call(lib, kind=TR.PS, flags=_lib.FX_FLAG_INIT, null=None, stable_sent=True, n=3, thr=2, steps=8, keys=4):
    """fx_table_advance over host arrays (no launch happens without a device)."""
    S, vmax = 2, 1
    pw = _lib.plane_words(S, steps)
    arr = {nm: np.zeros(pw, np.uint32) for nm in ("hdr", "dot", "clock", "votes3", "nkeys", "order", "release", "sent")}
    arr["votes3"] = np.zeros(3 * pw, np.uint32)
    small = {nm: np.zeros(S, np.uint32) for nm in ("nexec", "err")}
    state = np.zeros(max(lib.fx_table_session_bytes(min(kind, 2), n, keys, S), 4) // 4, np.uint32)
    ptr = lambda nm, a: None if null == nm else a.ctypes.data
    base = _lib.TableBatch(ptr("hdr", arr["hdr"]), ptr("dot", arr["dot"]), ptr("clock", arr["clock"]),
                           ptr("votes", arr["votes3"]), None, S, steps, n, keys, vmax, thr)
    inb = _lib.TableBatchMk(base, ptr("nkeys", arr["nkeys"]))
    outb = _lib.OrderBatch(ptr("order", arr["order"]), ptr("release", arr["release"]), ptr("nexec", small["nexec"]),
                           ptr("err", small["err"]))
    return lib.fx_table_advance(None if null == "in" else ctypes.byref(inb), kind,
                                None if null == "out" else ctypes.byref(outb), None,
                                arr["sent"].ctypes.data if stable_sent else None, ptr("state", state), flags, None)


def test_advance_argument_checks_come_before_the_device_check(lib):
    bad = _lib.FX_ERR_INVALID_ARG
    assert call(lib, kind=3) == bad
    for flags in (4, 8, _lib.FX_FLAG_INIT | _lib.FX_FLAG_SAVE_STATE, 1 << 8):
        assert call(lib, flags=flags) == bad
    for null in ("in", "out", "hdr", "dot", "clock", "votes", "nkeys", "order", "release", "nexec", "err", "state"):
        assert call(lib, null=null) == bad, null
    assert call(lib, kind=TR.MK, null="nkeys", stable_sent=False) == bad
    assert call(lib, kind=TR.MK) == bad and call(lib, kind=TR.SINGLE) == bad  # stable_sent is _ps's
    assert call(lib, n=17, thr=2) == bad and call(lib, thr=4) == bad and call(lib, thr=0) == bad
    assert call(lib, steps=1 << 26) == bad and call(lib, keys=0) == bad


def test_advance_without_a_device(lib):
    if lib.fx_device_count() > 0:
        pytest.skip("a GPU is visible")
    no = _lib.FX_ERR_NO_DEVICE
    assert call(lib) == no and call(lib, stable_sent=False) == no
    assert call(lib, flags=0) == no and call(lib, flags=_lib.FX_FLAG_INIT | _lib.FX_FLAG_EXECUTE_AT_COMMIT) == no
    assert call(lib, kind=TR.MK, stable_sent=False) == no
    assert call(lib, kind=TR.SINGLE, stable_sent=False) == no
    assert call(lib, kind=TR.SINGLE, stable_sent=False, null="nkeys") == no  # nkeys may be NULL there


# -------------------------------------------------------- routing logic
def same(got, want):
    return all(got[f] == want[f] for f in TR.FIELDS)


@pytest.mark.parametrize("shards,n,f,conflict", [g + (c,) for g in TP.GROUPS for c in TP.CONFLICTS])
def test_closed_loop_reproduces_the_generated_groups(shards, n, f, conflict):
    """run_table_groups over the restatement, own events only going in, must
    hand back the streams synth_table_group(..., msg_lag = 0) built -- the "S"
    events in place -- and its results; every group of the configuration in
    one session."""
    thr = T.quorum_sizes(n, f, False)[2]
    gen = TP.generated(shards, n, f, conflict, msg_lag=0)
    made = []
    factory = lambda *a, **kw: made.append(TR.RefSession(*a, **kw)) or made[-1]
    out = ft.run_table_groups([(TR.own_events(sts), commands) for sts, commands, _ in gen], n, TP.KEYS, thr,
                              session=factory)
    assert len(out) == len(gen) == TP.SEEDS and len(made) == 1 and made[0].S == shards * TP.SEEDS
    for got, (sts, _, results) in zip(out, gen):
        assert got["streams"] == [list(st) for st in sts]
        assert all(same(g, w) for g, w in zip(got["results"], results))
        assert got["rounds"] >= max(len(st) for st in TR.own_events(sts))
    assert made[0].calls == max(g["rounds"] for g in out)  # one advance per round
    assert sum(ev[0] == "S" for g in out for st in g["streams"] for ev in st) > 20 * len(out)


@pytest.mark.parametrize("shards,n,f,conflict", [g + (c,) for g in TP.GROUPS for c in TP.CONFLICTS])
def test_closed_loop_with_delays(shards, n, f, conflict):
    """The same with every message 0..3 rounds late, against the closed loop
    restated event by event in tests/table_resume.py; with delay 0 that loop
    too gives the generated streams."""
    thr = T.quorum_sizes(n, f, False)[2]
    gen = TP.generated(shards, n, f, conflict, msg_lag=0)
    groups = [(TR.own_events(sts), commands) for sts, commands, _ in gen]
    out = ft.run_table_groups(groups, n, TP.KEYS, thr, delay=TR.hashed_delay, session=TR.RefSession)
    moved = 0
    for got, (own, commands), (sts, _, _) in zip(out, groups, gen):
        streams, results = TR.closed_loop(own, commands, n, thr, TP.KEYS, TR.hashed_delay)
        assert got["streams"] == streams and all(same(g, w) for g, w in zip(got["results"], results))
        assert TP.s_events(streams) == TP.s_events(sts)  # the same messages, at other rows
        moved += streams != [list(st) for st in sts]
        assert all(r["err"] == 0 for r in results)
    assert moved == len(gen)
    streams, _ = TR.closed_loop(groups[0][0], groups[0][1], n, thr, TP.KEYS)
    assert streams == [list(st) for st in gen[0][0]]


def test_closed_loop_with_a_stream_that_stops():
    """Shard 1's stream is the hand-written count_above_missing (two messages
    for a two-shard command): it stops with FX_ERR_INVALID_ARG, the messages
    to it are dropped and shard 0 finishes."""
    own = [[TP.att(0, TP.S1, 1, 1, 1, 1), ("D", 0, [(3, 1, 1)]), ("D", 2, [(3, 1, 1)]), ("D", 2, [(3, 2, 2)]),
            TP.att(1, TP.Y, 2, 1, 1, 2)],  # Y is stable at shard 0 in round 4: shard 1 stopped in round 3
           list(TP.HAND["count_above_missing"][0])]
    commands = {TP.Y: {0: [1], 1: [2]}}
    out = ft.run_table_groups([(own, commands)], TP.HAND_N, TP.HAND_KEYS, TP.HAND_THR, session=TR.RefSession)[0]
    assert [r["err"] for r in out["results"]] == [0, _lib.FX_ERR_INVALID_ARG]
    assert out["streams"][0] == own[0] and out["results"][0]["sent"] == {4: 4}
    assert out["streams"][1] == own[1] and out["results"][1]["order"] == [0]  # the message to it was dropped
    streams, results = TR.closed_loop(own, commands, TP.HAND_N, TP.HAND_THR, TP.HAND_KEYS)
    assert streams == out["streams"] and all(same(g, w) for g, w in zip(out["results"], results))


def test_capacity_of_the_planes():
    """One row per own event and per (key here, other shard) of a multi-shard command."""
    seen = []

    class Spy(TR.RefSession):
        def __init__(self, S, steps, *rest, **kw):
            seen.append((S, steps))
            super().__init__(S, steps, *rest, **kw)

    sts, commands, _ = TP.generated(3, 3, 1, 100, msg_lag=0)[0]
    own = TR.own_events(sts)
    out = ft.run_table_groups([(own, commands)], 3, TP.KEYS, 2, session=Spy)[0]
    cap = [len(own[g]) + sum(len(c[g]) * (len(c) - 1) for c in commands.values() if g in c) for g in range(3)]
    assert seen == [(3, max(cap))] and [len(st) for st in out["streams"]] == cap  # every message arrived


# ------------------------------------------- the inputs of the GPU cut tests
@pytest.mark.parametrize("kind", KINDS)
def test_cut_streams_hold_what_the_cuts_need(kind):
    st, thr = TR.cut_stream(kind)
    assert 150 <= len(st) <= 300
    pre = TR.prefixes(kind, st, TR.CUT_N, thr, TR.CUT_KEYS)
    assert len(pre) == len(st) + 1 and pre[-1][1] == 0 and pre[-1][0] > 40
    if kind == TR.SINGLE:
        return
    left, four, pairs = TR.coverage(st, TR.CUT_N, thr, TR.CUT_KEYS)
    assert len(left) >= 3 and len(four) >= 1  # (coverage() leaves the last event out)
    if kind == TR.PS:
        assert len(pairs) >= 1
