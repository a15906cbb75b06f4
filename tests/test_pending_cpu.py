"""The pending stage without a device: the host twin (fx_pending_aggregate_host)
against the restatement of aggregate.rs (pending_ref) on every shape and both
tiers, the reference's pending_flow test as recorded rows, and the join with
the KV stage's results (command_results) behind the table executor's
restatement."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import kv as K
from fantoch_amd import pending as P
from fantoch_amd import table as ft

import kv_shapes as KS
import pending_ref
import pending_shapes as PS

CASES = PS.all_cases()
RUNS = [(i, t) for i, c in enumerate(CASES) for t in c.tiers if t is not None]


@pytest.mark.parametrize("i,tier", RUNS, ids=["%s tier%d" % (CASES[i].name, t) for i, t in RUNS])
def test_host_twin_equals_restatement(i, tier):
    case = CASES[i]
    case.check(case.run_host(tier), tier)


def test_the_shapes_reach_their_edges():
    """What the names of the shapes promise, on the restatement alone."""
    cap = PS.capacity()
    peaks = [cap.restated(s, PS.HBM)["peak"] for s in range(cap.S)]
    assert peaks[0] == 64 and peaks[1] == 65 and peaks[3] == 64 and peaks[4] == 65 and peaks[5] == 64
    stop = cap.restated(1, PS.ONCHIP)
    assert stop["err"] == PS.C and stop["nopen"] == 64 and max(stop["head"]) == 63
    hb = PS.hbm_buckets()
    buckets = _lib.pending_buckets(hb.steps)
    for s, bucket in ((0, 1), (1, buckets - 1)):
        firsts = hb.streams[s]["rifl_of"][:70]
        assert len(set(firsts)) == 70 and {_lib.pending_bucket(r, buckets) for r in firsts} == {bucket}
    wide = PS.pairs_and_wide()
    ref = wide.restated(4, PS.HBM)
    assert ref["ready"].count(10) == 1 and [ref["part"][(j, 10)] for j in range(8)] == [10, 40, 63, 64, 70, 127, 128, 140]
    assert [h for h in wide.restated(5, PS.HBM)["ready"] if h < 3] == [2, 1, 0]


def test_bucket_function_and_state_size(lib):
    rng = random.Random(1)
    for _ in range(2000):
        r, b = rng.randrange(1 << 32), rng.choice([1, 2, 3, 7, 64, 1000, rng.randrange(1, 1 << 20)])
        assert lib.fx_pending_bucket(r, b) == _lib.pending_bucket(r, b) < b
    for steps, lanes in ((0, 1), (1, 1), (64, 2), (65, 3), (1000, 5)):
        assert lib.fx_pending_state_bytes(steps, lanes) == lanes * _lib.pending_buckets(steps) * 64 * 16
        assert _lib.pending_buckets(steps) * 64 >= steps


def test_refused_calls_write_nothing(lib):
    case = PS.reuse()
    for kw in (dict(count_mask=0), dict(tier=2)):
        args = dict(count_mask=0xFF, tier=PS.HBM)
        args.update(kw)
        res = P.run_pending_host(case.order, case.nexec, case.rifl, case.count, case.S, case.steps, fill=0xA5, **args)
        assert res.status == _lib.FX_ERR_INVALID_ARG
        assert all(np.all(getattr(res, name) == PS.A5) for name in P.NAMES)
    assert lib.fx_pending_aggregate_host(None, None, 0) == _lib.FX_ERR_INVALID_ARG
    assert lib.fx_pending_aggregate(None, None, None, 0, 0, None, None) == _lib.FX_ERR_INVALID_ARG
    assert lib.fx_pending_run(None, None, None, None) == _lib.FX_ERR_INVALID_ARG
    if lib.fx_device_count() <= 0:  # no fallback to the host twin behind the device calls
        z = np.zeros(_lib.plane_words(1, 4) * 8, np.uint32)
        inb = _lib.PendingBatch(*[z.ctypes.data] * 4, 0xFF, 0, 1, 4)
        outb = _lib.PendingOut(*[z.ctypes.data] * 7)
        assert lib.fx_pending_run(ctypes.byref(inb), ctypes.byref(outb), None, None) == _lib.FX_ERR_NO_DEVICE
        assert lib.fx_pending_aggregate(ctypes.byref(inb), ctypes.byref(outb), None, 1, 0, None, None) == \
            _lib.FX_ERR_NO_DEVICE


def test_pending_flow_of_the_reference():
    """aggregate.rs:96-209: put_a -> [None], put_b -> [None], get_ab -> {A: [Some(foo)], B: [None]}, in that order."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pending_kat.json")) as f:
        kat = json.load(f)
    rows = kat["rows"]
    steps = len(rows)
    at = _lib.index(np.arange(steps), 0, steps)
    pw = _lib.plane_words(1, steps)
    order, rifl, key, count, ops = (np.full(pw, PS.A5, np.uint32) for _ in range(5))
    order[at] = np.arange(steps)
    rifl[at], key[at], count[at] = ([r[name] for r in rows] for name in ("rifl", "key", "count"))
    ops[at] = [K.kv_op(*r["op"]) for r in rows]
    kv = K.run_kv_host(order, [steps], key, ops, 1, steps, 2, 1, fill=0xA5)
    res = P.run_pending_host(order, [steps], rifl, count, 1, steps, fill=0xA5)
    assert res.status == 0 and int(res.err[0]) == 0 and int(kv.err[0]) == 0
    assert [int(h) for h in res.head[at]] == kat["heads"]
    assert res.ready_heads(0) == kat["ready"] and int(res.nopen[0]) == 0
    got = [(kat["names"][str(r)], {str(k): v for k, v in per_key.items()})
           for r, per_key in P.command_results(res, kv, key, 0)]
    assert got == [(name, per_key) for name, per_key in kat["results"]]
    assert got[2] == ("get_ab", {"0": [1], "1": [None]})


def test_command_results_behind_the_table_executor():
    """Every command of KS.table_batch(True) executes (check_precondition), so nothing stays open, there is one
    result per distinct dot, and the four replicas of a group give every command the same per-key results."""
    batch = KS.table_batch(True)
    KS.check_precondition(batch)
    planes = ft.pack_table_streams([b[0] for b in batch], KS.N, KS.KEYS)
    ops, omax = K.pack_kv_ops([b[3] for b in batch], planes.steps, omax=2)
    S, steps = planes.S, planes.steps
    order = np.full(planes.plane, PS.A5, np.uint32)
    nexec = np.zeros(S, np.uint32)
    for s, (ev, ref, keys_of, ops_of) in enumerate(batch):
        nexec[s] = len(ref["order"])
        order[_lib.index(np.arange(len(ref["order"])), s, steps)] = ref["order"]
    kv = K.run_kv_host(order, nexec, planes.hdr, ops, S, steps, KS.KEYS, omax, 0x00FFFFFF, fill=0xA5)
    res = P.run_pending_host(order, nexec, planes.dot, planes.nkeys, S, steps, fill=0xA5)
    assert res.status == 0 and np.all(res.err == 0) and np.all(kv.err == 0)
    per_stream = []
    for s, (ev, ref, keys_of, ops_of) in enumerate(batch):
        dots = {e[2] for e in ev if e[0] == "A"}
        assert int(res.nopen[s]) == 0 and int(res.nready[s]) == len(dots)
        got = P.command_results(res, kv, planes.hdr, s, key_mask=0x00FFFFFF, ops=ops)
        assert len({r for r, _ in got}) == len(got) == len(dots)
        for r, per_key in got:  # one entry per key of the command, as many results as the partial has ops
            want = {e[1]: len(o) for e, o in zip(ev, ops_of) if e[0] == "A" and _lib.pack_dot(*e[2]) == r}
            assert {k: len(v) for k, v in per_key.items()} == want
        per_stream.append(dict(got))
    assert any(len(v) == 2 for v in per_stream[0].values())
    for g in range(0, S, 4):
        for s in range(g + 1, g + 4):
            assert per_stream[s] == per_stream[g]


def test_command_results_do_not_depend_on_the_fill():
    """The default fill is 0, which is also a head row: a command whose head is row 0, in a stream with rows
    that never execute, has the partials its count says and no more, whatever the outputs held before."""
    X, Y = PS.rifl(7), PS.rifl(8, 2)
    steps = 12
    at = _lib.index(np.arange(steps), 0, steps)
    pw = _lib.plane_words(1, steps)
    order, rifl, key, count, ops = (np.full(pw, PS.A5, np.uint32) for _ in range(5))
    executed = [0, 5, 1]  # rows 2 .. 4 and 6 .. 11 never execute (votes, stable events)
    order[at[:3]] = executed
    rifl[at[[0, 1, 5]]], count[at[[0, 1, 5]]], key[at[[0, 1, 5]]] = [X, X, Y], [2, 2, 1], [0, 1, 1]
    ops[at] = K.kv_op(K.EMPTY)
    ops[at[[0, 1, 5]]] = [K.kv_op(K.PUT, 3), K.kv_op(K.GET), K.kv_op(K.PUT, 4)]
    want = [(Y, {1: [None]}), (X, {0: [None], 1: [4]})]
    for fill in (None, 0, 0xA5, 0xFF):
        kw = {} if fill is None else dict(fill=fill)
        kv = K.run_kv_host(order, [3], key, ops, 1, steps, 2, 1, **kw)
        res = P.run_pending_host(order, [3], rifl, count, 1, steps, **kw)
        assert int(res.err[0]) == 0 and res.ready_heads(0) == [5, 0] and res.members(0, 0) == 2
        assert P.command_results(res, kv, key, 0, ops=ops) == want
    # the same over an executor's output, where most rows are votes that never execute
    batch = KS.table_batch(True)[:4]
    planes = ft.pack_table_streams([b[0] for b in batch], KS.N, KS.KEYS)
    ops, omax = K.pack_kv_ops([b[3] for b in batch], planes.steps, omax=2)
    S, steps = planes.S, planes.steps
    order, nexec = np.zeros(planes.plane, np.uint32), np.zeros(S, np.uint32)
    for s, (ev, ref, keys_of, ops_of) in enumerate(batch):
        nexec[s] = len(ref["order"])
        order[_lib.index(np.arange(len(ref["order"])), s, steps)] = ref["order"]
    got = []
    for kw in ({}, dict(fill=0xA5)):
        kv = K.run_kv_host(order, nexec, planes.hdr, ops, S, steps, KS.KEYS, omax, 0x00FFFFFF, **kw)
        res = P.run_pending_host(order, nexec, planes.dot, planes.nkeys, S, steps, **kw)
        got.append([P.command_results(res, kv, planes.hdr, s, key_mask=0x00FFFFFF, ops=ops) for s in range(S)])
    assert got[0] == got[1] and all(len(g) == int(n) for g, n in zip(got[0], res.nready))
    assert any(e[0] != "A" for e in batch[0][0])
