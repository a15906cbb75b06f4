"""The KV stage without a GPU: the host twins (fx_kv_execute_host,
fx_kv_monitor_compare_host, fx_kv_synth_ops_host) against the restatement of
kvs.rs and monitor.rs (kv_ref), the struct layouts against the header, every
refusal, and the stand-alone sanitizer run of the host twins.  CPU only."""
import ctypes
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import kv as K

import kv_ref
import kv_shapes as KS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A5 = KS.A5
MASK64 = (1 << 64) - 1


# ------------------------------------------------------------------ semantics
def test_store_flow_kat():
    """kvs.rs:91-158, one op per execute, through the restatement and the host twin."""
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kvs_kat.json")))["steps"]
    key_id = {"A": 0, "B": 1}
    val_id = {None: 0, "x": 1, "y": 2, "z": 3}
    words = {"get": lambda v: K.kv_op(K.GET), "put": lambda v: K.kv_op(K.PUT, val_id[v]),
             "delete": lambda v: K.kv_op(K.DELETE)}
    keys_of = [key_id[st["key"]] for st in kat]
    ops_of = [[words[st["op"]](st["value"])] for st in kat]
    want = [val_id[st["expect"]] for st in kat]
    order = list(range(len(kat)))
    results, store, monitor = kv_ref.run(order, keys_of, ops_of)
    assert [results[a][0] for a in order] == want and store == {}
    ops, omax = K.pack_kv_ops([ops_of], len(kat))
    assert omax == 1
    order_p = np.zeros(_lib.plane_words(1, len(kat)), np.uint32)  # a stream's rows are not a plane's first words
    key_p = np.zeros(len(order_p), np.uint32)
    idx = _lib.index(np.arange(len(kat)), 0, len(kat))
    order_p[idx], key_p[idx] = order, keys_of
    res = K.run_kv_host(order_p, [len(kat)], key_p, ops, 1, len(kat), 2, 1)
    assert [res.results(0, a)[0] for a in order] == want
    kv_ref.check_stream(res, 0, order, keys_of, ops_of)
    assert K.monitor_rows(res, 0, 0) == [a for a in order if keys_of[a] == 0 and kat[a]["op"] != "get"]


def test_put_returns_none_and_delete_returns_the_value():
    r, store, mon = kv_ref.run([0, 1, 2, 3], [0] * 4, [[KS.P(5)], [KS.P(6)], [KS.D], [KS.D]])
    assert r == {0: [0], 1: [0], 2: [6], 3: [0]} and store == {} and mon == {0: [0, 1, 2, 3]}


@pytest.mark.parametrize("case", KS.all_cases(), ids=lambda c: c.name)
def test_host_twin_matches_the_restatement(case):
    case.check(case.run_host())


def test_pack_kv_ops():
    ops, omax = K.pack_kv_ops([[[KS.G], [], [KS.P(3), KS.D]], [[KS.D]]], 3)
    pw = _lib.plane_words(2, 3)
    E = K.kv_op(K.EMPTY)
    assert omax == 2 and len(ops) == 2 * pw and K.kv_op(K.PUT, 3) == 0x40000003 and E == 0xC0000000
    at = lambda s, a: int(_lib.index(a, s, 3))
    assert [int(ops[at(0, a)]) for a in range(3)] == [KS.G, E, KS.P(3)]
    assert [int(ops[pw + at(0, a)]) for a in range(3)] == [E, E, KS.D]
    assert int(ops[at(1, 0)]) == KS.D and int(ops[at(1, 1)]) == E
    with pytest.raises(ValueError):
        K.pack_kv_ops([[[KS.G] * 5]], 1)


@pytest.mark.parametrize("mk", [False, True], ids=["single-key", "kmax2"])
def test_table_restatement_then_host_twin(mk):
    """The end-to-end case of the GPU tests with the table executor's restatement in its place."""
    from fantoch_amd import table as ft
    batch = KS.table_batch(mk)
    KS.check_precondition(batch)
    planes = ft.pack_table_streams([b[0] for b in batch], KS.N, KS.KEYS)
    ops, omax = K.pack_kv_ops([b[3] for b in batch], planes.steps, omax=2)
    order = np.full(planes.plane, A5, np.uint32)
    for s, b in enumerate(batch):
        order[_lib.index(np.arange(b[1]["nexec"]), s, planes.steps)] = b[1]["order"]
    res = K.run_kv_host(order, [b[1]["nexec"] for b in batch], planes.hdr, ops, planes.S, planes.steps, KS.KEYS, omax,
                        0x00FFFFFF, fill=0xA5)
    for s, (ev, ref, keys_of, ops_of) in enumerate(batch):
        kv_ref.check_stream(res, s, ref["order"], keys_of, ops_of)
    pairs = [(g, g + r) for g in range(0, len(batch), 4) for r in range(1, 4)]
    assert K.compare_monitors_host(res, planes.dot, res, planes.dot, pairs) == [(_lib.FX_KV_AGREE,) * 2] * len(pairs)


# ------------------------------------------------------------------ C ABI
PAIRS = {"KvBatch": "fx_kv_batch", "KvOut": "fx_kv_out", "KvMonitor": "fx_kv_monitor"}
CONSTS = ["FX_KV_GET", "FX_KV_PUT", "FX_KV_DELETE", "FX_KV_EMPTY", "FX_KV_MAX_OPS", "FX_KV_AGREE", "FX_KV_BAD_PAIR",
          "FX_KV_ONCHIP_KEYS"]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ctypes_mirrors_match_the_header():
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "fantoch_amd.h"', "int main(void) {"]
    for py, c in PAIRS.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (py, c))
        for name, _ in getattr(_lib, py)._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (py, name, c, name))
    for name in CONSTS:
        lines.append('  printf("C %s %%u\\n", (unsigned)%s);' % (name, name))
    lines.append('  printf("C op %u\\n", (unsigned)FX_KV_OP(FX_KV_DELETE, 0x7FFFFFFFu));')
    lines += ["  return 0;", "}"]
    d = tempfile.mkdtemp()
    try:
        src, exe = os.path.join(d, "abi.c"), os.path.join(d, "abi")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True,
                       capture_output=True, text=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    finally:
        shutil.rmtree(d, ignore_errors=True)
    layout = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out.split("\n") if ln}
    for py in PAIRS:
        cls = getattr(_lib, py)
        assert ctypes.sizeof(cls) == layout[(py, "size")], py
        for name, _ in cls._fields_:
            assert getattr(cls, name).offset == layout[(py, name)], (py, name)
    for name in CONSTS:
        assert layout[("C", name)] == getattr(_lib, name), name
    assert layout[("C", "op")] == K.kv_op(K.DELETE, 0x7FFFFFFF) == 0xBFFFFFFF


def test_symbols_are_bound(lib):
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for name in ("fx_kv_execute", "fx_kv_execute_host", "fx_kv_monitor_compare", "fx_kv_monitor_compare_host",
                 "fx_kv_synth_ops", "fx_kv_synth_ops_host"):
        assert hasattr(lib, name) and name in bound


# ------------------------------------------------------------------ refusals
def small_call():
    case = KS.op_slots(2)
    pw = case.plane
    bufs = dict(order=case.order, nexec=case.nexec, key=case.key, ops=case.ops,
                result=np.full(2 * pw, A5, np.uint32), store=np.full(case.S * case.keys, A5, np.uint32),
                monitor=np.full(pw, A5, np.uint32), mon_off=np.full(case.S * (case.keys + 1), A5, np.uint32),
                err=np.full(case.S, A5, np.uint32))
    return case, bufs


def call_execute(lib, case, bufs, fn="fx_kv_execute_host", **over):
    p = {k: v.ctypes.data for k, v in bufs.items()}
    f = dict(S=case.S, steps=case.steps, keys=case.keys, omax=case.omax)
    for k, v in over.items():
        (p if k in p else f)[k] = v
    inb = _lib.KvBatch(p["order"], p["nexec"], p["key"], case.key_mask, p["ops"], f["S"], f["steps"], f["keys"],
                       f["omax"])
    outb = _lib.KvOut(p["result"], p["store"], p["monitor"], p["mon_off"], p["err"])
    extra = () if fn.endswith("_host") else (None,)
    return getattr(lib, fn)(ctypes.byref(inb), ctypes.byref(outb), *extra)


@pytest.mark.parametrize("fn", ["fx_kv_execute_host", "fx_kv_execute"])
def test_refused_calls_write_nothing(lib, fn):
    case, bufs = small_call()
    outs = ("result", "store", "monitor", "mon_off", "err")
    refused = [dict(omax=0), dict(omax=_lib.FX_KV_MAX_OPS + 1), dict(keys=0), dict(keys=_lib.FX_TABLE_MAX_KEYS + 1)]
    refused += [{name: None} for name in ("order", "nexec", "key", "ops") + outs]
    for over in refused:
        assert call_execute(lib, case, bufs, fn, **over) == _lib.FX_ERR_INVALID_ARG, over
        for name in outs:
            assert np.all(bufs[name] == A5), (over, name)
    extra = () if fn.endswith("_host") else (None,)
    assert getattr(lib, fn)(None, None, *extra) == _lib.FX_ERR_INVALID_ARG


def test_device_calls_need_a_device(lib):
    if lib.fx_device_count() > 0:
        pytest.skip("a GPU is visible")
    case, bufs = small_call()
    assert call_execute(lib, case, bufs, "fx_kv_execute") == _lib.FX_ERR_NO_DEVICE
    assert np.all(bufs["err"] == A5)
    ops = np.zeros(256, np.uint32)
    assert lib.fx_kv_synth_ops(1, 0, 10, 10, None, 1, 4, ops.ctypes.data, None) == _lib.FX_ERR_NO_DEVICE
    res = case.run_host()
    m = _lib.KvMonitor(res.monitor.ctypes.data, res.mon_off.ctypes.data, case.key.ctypes.data, case.S, case.steps,
                       case.keys)
    pairs, diff = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    assert lib.fx_kv_monitor_compare(ctypes.byref(m), ctypes.byref(m), pairs.ctypes.data, 1, diff.ctypes.data,
                                     None) == _lib.FX_ERR_NO_DEVICE


def test_an_empty_batch_is_fine(lib):
    case, bufs = small_call()
    assert call_execute(lib, case, bufs, S=0) == 0
    assert all(np.all(bufs[n] == A5) for n in ("result", "store", "monitor", "mon_off", "err"))


# ------------------------------------------------------------------ monitors
def monitored():
    """Three streams on 4 keys: 0 and 1 execute the same commands per key in the same per-key order
    (interleaved otherwise, arriving in other rows), 2 differs."""
    names = [100 + i for i in range(12)]
    keyof = {n: i % 4 for i, n in enumerate(names)}
    sts, rifls = [], []
    for perm, exec_order in (([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]),
                             ([11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0], [3, 2, 1, 0, 7, 6, 5, 4, 11, 10, 9, 8]),
                             ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [0, 1, 2, 3, 4, 9, 6, 7, 8, 5, 10, 11])):
        arrived = [names[i] for i in perm]
        sts.append(KS.stream([arrived.index(names[i]) for i in exec_order], [keyof[n] for n in arrived],
                             [[KS.G] if n == 103 else [KS.P(n)] for n in arrived]))
        rifls.append(arrived)
    case = KS.Case("monitored", sts, 4, 1)
    rifl = np.full(case.plane, A5, np.uint32)
    for s, arrived in enumerate(rifls):
        rifl[_lib.index(np.arange(12), s, case.steps)] = arrived
    return case, rifl


def test_monitor_compare_host():
    case, rifl = monitored()
    res = case.run_host()
    case.check(res)
    AG = _lib.FX_KV_AGREE
    got = K.compare_monitors_host(res, rifl, res, rifl, [(0, 1), (1, 0), (0, 0), (0, 2), (2, 1), (3, 0), (0, 7)])
    assert got[:3] == [(AG, AG)] * 3
    assert got[3] == got[4] == (1, 1)  # key 1: 101, 105, 109 against 101, 109, 105
    assert got[5] == got[6] == (_lib.FX_KV_BAD_PAIR,) * 2
    # a key that ends early: the difference is at the shorter length; the smaller key wins
    short = case.run_host()
    short.mon_off[2, 3:] -= 1  # stream 2 loses the last row of key 2
    m = short.monitor
    for r in range(int(short.mon_off[2, 3]), int(short.mon_off[2, 4])):
        m[_lib.index(r, 2, case.steps)] = m[_lib.index(r + 1, 2, case.steps)]
    assert K.compare_monitors_host(res, rifl, short, rifl, [(2, 2), (0, 2)]) == [(2, 2), (1, 1)]
    # a stream that ended with an error (its rows as the caller filled them) cannot be compared
    bad = KS.errors(64)
    rb = bad.run_host()
    assert K.compare_monitors_host(rb, bad.key, rb, bad.key, [(0, 1), (0, 0)]) == \
        [(_lib.FX_KV_BAD_PAIR,) * 2, (AG, AG)]


def test_monitor_compare_refusals(lib):
    case, rifl = monitored()
    res = case.run_host()
    off = np.ascontiguousarray(res.mon_off)
    diff, pairs = np.full(2, A5, np.uint32), np.zeros(2, np.uint32)

    def call(a_keys=4, b_keys=4, mon=res.monitor.ctypes.data, rf=rifl.ctypes.data, pr=pairs.ctypes.data,
             df=diff.ctypes.data, n=1):
        a = _lib.KvMonitor(mon, off.ctypes.data, rf, 3, case.steps, a_keys)
        b = _lib.KvMonitor(res.monitor.ctypes.data, off.ctypes.data, rifl.ctypes.data, 3, case.steps, b_keys)
        return lib.fx_kv_monitor_compare_host(ctypes.byref(a), ctypes.byref(b), pr, n, df)

    for kw in (dict(a_keys=3), dict(a_keys=0, b_keys=0), dict(mon=None), dict(rf=None), dict(pr=None), dict(df=None)):
        assert call(**kw) == _lib.FX_ERR_INVALID_ARG, kw
        assert np.all(diff == A5)
    assert call(pr=None, df=None, n=0) == 0
    assert call() == 0 and list(diff) == [_lib.FX_KV_AGREE] * 2


# ------------------------------------------------------------------ op generator
def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def draw(seed, g, a, purpose):
    return mix64((mix64((mix64(seed ^ 0x5851F42D4C957F2D) + g) & MASK64) + (a << 8) + purpose) & MASK64)


def synth_op(seed, g, row, read_pct, delete_pct):
    d = draw(seed, g, row, 16)
    p = (d >> 32) % 100
    if p < read_pct:
        return K.kv_op(K.GET)
    if p < read_pct + delete_pct:
        return K.kv_op(K.DELETE)
    return K.kv_op(K.PUT, 1 + d % ((1 << 30) - 1))


def test_op_generator_matches_the_draw():
    S, steps, base = 67, 9, 1 << 20
    lengths = [(7 * s) % (steps + 1) for s in range(S)]
    ops = K.synth_kv_ops_host(5, S, steps, 30, 20, lengths, stream_base=base)
    E = K.kv_op(K.EMPTY)
    want = np.full(_lib.plane_words(S, steps), E, np.uint32)
    for s in range(S):
        for r in range(lengths[s]):
            want[_lib.index(r, s, steps)] = synth_op(5, base + s, r, 30, 20)
    assert np.array_equal(ops, want)
    kinds = np.bincount(K.synth_kv_ops_host(9, 64, 400, 30, 20) >> 30, minlength=4)
    assert kinds[3] == 0 and abs(kinds[0] / 25600 - 0.3) < 0.02 and abs(kinds[2] / 25600 - 0.2) < 0.02
    assert np.all(K.synth_kv_ops_host(9, 3, 5, 100, 0, None)[_lib.index(np.arange(5), 2, 5)] == K.kv_op(K.GET))
    full = K.synth_kv_ops_host(5, S, steps, 30, 20, None, stream_base=base)  # a stream does not depend on its length
    assert all(full[_lib.index(r, s, steps)] == want[_lib.index(r, s, steps)] for s in range(S)
               for r in range(lengths[s]))


def test_op_generator_refusals(lib):
    ops = np.full(256, A5, np.uint32)
    for args in ((1, 0, 101, 0), (1, 0, 60, 41), (1, 0, 0, 101), (1, 0xFFFFFFFF, 0, 0)):
        assert lib.fx_kv_synth_ops_host(*args, None, 2, 4, ops.ctypes.data) == _lib.FX_ERR_INVALID_ARG
        assert np.all(ops == A5)
    assert lib.fx_kv_synth_ops_host(1, 0, 0, 0, None, 2, 4, None) == _lib.FX_ERR_INVALID_ARG


# ------------------------------------------------------------------ sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_twins_under_the_sanitizers():
    out = subprocess.run(["make", "-C", ROOT, "kv-check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "kv_host_check: ok" in out.stdout
