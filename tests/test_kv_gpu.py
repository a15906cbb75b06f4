"""The KV stage on the device (fx_kv_execute, fx_kv_monitor_compare,
fx_kv_synth_ops): every output byte against the host twin, and both against
the restatement of kvs.rs and monitor.rs (kv_ref); behind the table executor
and a graph executor end to end.  Every buffer starts as 0xA5 bytes and the
register file is filled with garbage before the launches.  GPU only."""
import os
import sys

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import kv as K
from fantoch_amd import streams as fs
from fantoch_amd import table as ft

import kv_ref
import kv_shapes as KS
import table_ref as R
from test_sim_poison import FILLS, poisoner

pytestmark = pytest.mark.gpu

AGREE = (_lib.FX_KV_AGREE, _lib.FX_KV_AGREE)
CASES = KS.all_cases()


def same_bytes(dev, host):
    for name in ("err", "result", "store", "monitor", "mon_off"):
        a, b = getattr(dev, name), getattr(host, name)
        assert np.array_equal(a, b), "%s differs at word %d" % (name, int(np.flatnonzero(a.ravel() != b.ravel())[0]))


def run_case(case, fill=FILLS[0], **kw):
    return fd.run_kv(case.order, case.nexec, case.key, case.ops, case.S, case.steps, case.keys, case.omax,
                     case.key_mask, fill=0xA5, before_launch=poisoner(*fill), **kw)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.name for c in CASES])
def test_device_equals_host_twin_and_restatement(gpu, i):
    """Chunk edges (nexec 0 / 1 / 63 / 64 / 65 / 129, S 1 / 64 / 65), the row patterns and the monitor
    on both table tiers, the op slots, the order word's flag, every per-stream status."""
    case = CASES[i]
    dev = run_case(case, FILLS[i % len(FILLS)])
    same_bytes(dev, case.run_host())
    case.check(dev)


def test_every_fill_of_the_register_file(gpu):
    case = KS.chunk_edges(65, KS.ABOVE, omax=4)
    host = case.run_host()
    case.check(host)
    for fill in FILLS:
        same_bytes(run_case(case, fill), host)


# ------------------------------------------------------------------ table -> KV
N, FQ, THR, KEYS = KS.N, KS.FQ, KS.THR, KS.KEYS
CMDS, LAG, WINDOW = KS.CMDS, KS.LAG, KS.WINDOW
table_batch, check_precondition = KS.table_batch, KS.check_precondition


@pytest.mark.parametrize("mk", [False, True], ids=["single-key", "kmax2"])
def test_table_then_kv(gpu, mk):
    batch = table_batch(mk)
    check_precondition(batch)
    planes = ft.pack_table_streams([b[0] for b in batch], N, KEYS)
    ops, omax = K.pack_kv_ops([b[3] for b in batch], planes.steps, omax=2)
    tab = fd.run_table(planes, THR, keep_device=True, order_fill=0xA5)
    assert np.all(tab.err == 0)
    # the executor's outputs and its hdr plane are read where they are
    res = fd.run_kv(tab.dev["order"], tab.dev["nexec"], tab.dev["hdr"], ops, planes.S, planes.steps, KEYS, omax,
                    key_mask=0x00FFFFFF, fill=0xA5, before_launch=poisoner(*FILLS[1]), keep_device=True)
    same_bytes(res, K.run_kv_host(tab.order, tab.nexec, planes.hdr, ops, planes.S, planes.steps, KEYS, omax,
                                  0x00FFFFFF, fill=0xA5))
    for s, (ev, ref, keys_of, ops_of) in enumerate(batch):
        kv_ref.check_stream(res, s, ref["order"], keys_of, ops_of)
    pairs = [(g, g + r) for g in range(0, len(batch), 4) for r in range(1, 4)]
    assert fd.compare_monitors(res, tab.dev["dot"], res, tab.dev["dot"], pairs) == [AGREE] * len(pairs)
    assert K.compare_monitors_host(res, planes.dot, res, planes.dot, pairs) == [AGREE] * len(pairs)
    for a, b in pairs:
        assert np.array_equal(res.store[a], res.store[b])


def test_device_streams_never_leave_the_device(gpu):
    """fx_table_synth_generate -> fx_table_run -> fx_kv_synth_ops -> fx_kv_execute over DeviceBuffers only."""
    p = ft.table_synth_params(seed=3, streams=65, n=5, fast_quorum=3, keys=16, cmds=30, conflicts=(2, 50), stream_base=7)
    t = fd.synth_table(p)
    tab = fd.run_table(t, THR, keep_device=True)
    assert np.all(tab.err == 0)
    ops = fd.synth_kv_ops(11, t.S, t.steps, 30, 20, lengths=t.lengths, stream_base=7)
    res = fd.run_kv(tab.dev["order"], tab.dev["nexec"], t.bufs["hdr"], ops, t.S, t.steps, 16, 1, key_mask=0x00FFFFFF,
                    fill=0xA5)
    host_planes = t.download()
    host_ops = K.synth_kv_ops_host(11, t.S, t.steps, 30, 20, host_planes.lengths, stream_base=7)
    assert np.array_equal(ops.download(np.uint32, t.plane), host_ops)
    same_bytes(res, K.run_kv_host(tab.order, tab.nexec, host_planes.hdr, host_ops, t.S, t.steps, 16, 1, 0x00FFFFFF,
                                  fill=0xA5))
    assert np.all(res.err == 0) and int(res.mon_off[:, 16].sum()) > 0
    for s in (0, 63, 64):
        order = [int(x) & 0x7FFFFFFF for x in tab.order[_lib.index(np.arange(int(tab.nexec[s])), s, t.steps)]]
        rows = _lib.index(np.arange(t.steps), s, t.steps)
        kv_ref.check_stream(res, s, order, [int(h) & 0xFFFFFF for h in host_planes.hdr[rows]],
                            [[int(o)] if K.op_kind(o) != K.EMPTY else [] for o in host_ops[rows]])


# ------------------------------------------------------------------ seeded disagreements
def all_put_replicas():
    """Two copies of one conflict-50 stream, every command a PUT, and the restatement's monitor."""
    ev = ft.synth_table_streams(2, N, FQ, KEYS, CMDS, 50, LAG, WINDOW)
    ref = R.run_stream(ev, N, THR, KEYS)
    keys_of = [e[1] for e in ev]
    ops_of = [[KS.P(1 + a)] if e[0] == "A" else [] for a, e in enumerate(ev)]
    planes = ft.pack_table_streams([ev, ev], N, KEYS)
    ops, _ = K.pack_kv_ops([ops_of, ops_of], planes.steps, omax=1)
    return ev, ref["order"], keys_of, planes, ops


def run_orders(planes, ops, orders):
    order = np.full(planes.plane, KS.A5, np.uint32)
    for s, o in enumerate(orders):
        order[_lib.index(np.arange(len(o)), s, planes.steps)] = o
    return fd.run_kv(order, [len(o) for o in orders], planes.hdr, ops, 2, planes.steps, KEYS, 1, key_mask=0x00FFFFFF,
                     fill=0xA5)


def test_seeded_disagreements(gpu):
    ev, order, keys_of, planes, ops = all_put_replicas()
    per_key = {k: [a for a in order if keys_of[a] == k] for k in range(KEYS)}
    # two adjacent order rows of one key (different dots) swapped
    i = next(i for i in range(len(order) - 1) if keys_of[order[i]] == keys_of[order[i + 1]] and
             ev[order[i]][2] != ev[order[i + 1]][2] and i > 3)
    key = keys_of[order[i]]
    swapped = order[:i] + [order[i + 1], order[i]] + order[i + 2:]
    res = run_orders(planes, ops, [order, swapped])
    want = (key, per_key[key].index(order[i]))
    assert fd.compare_monitors(res, planes.dot, res, planes.dot, [(0, 1), (1, 0), (0, 0)]) == [want, want, AGREE]
    assert K.compare_monitors_host(res, planes.dot, res, planes.dot, [(0, 1)]) == [want]
    # the last row of a key dropped: the difference is at the shorter length
    busy = sorted(k for k in per_key if len(per_key[k]) >= 2)
    assert len(busy) >= 2
    hi, lo = busy[-1], busy[0]
    drop_hi = [a for a in order if a != per_key[hi][-1]]
    res = run_orders(planes, ops, [order, drop_hi])
    assert fd.compare_monitors(res, planes.dot, res, planes.dot, [(0, 1), (1, 0)]) == [(hi, len(per_key[hi]) - 1)] * 2
    # differences at two keys: the smaller key is reported
    drop_both = [a for a in drop_hi if a != per_key[lo][-1]]
    res = run_orders(planes, ops, [order, drop_both])
    want = [(lo, len(per_key[lo]) - 1)]
    assert fd.compare_monitors(res, planes.dot, res, planes.dot, [(0, 1)]) == want
    assert K.compare_monitors_host(res, planes.dot, res, planes.dot, [(0, 1)]) == want


def test_pairs_that_cannot_be_compared(gpu):
    case = KS.errors(KS.ABOVE)
    res = run_case(case, keep_device=True)
    pairs = [(0, 0), (0, 1), (2, 0), (0, case.S), (4, 9)]
    got = fd.compare_monitors(res, case.key, res, case.key, pairs)
    BAD = (_lib.FX_KV_BAD_PAIR,) * 2
    assert got[0] == AGREE and got[1:4] == [BAD] * 3
    assert got == K.compare_monitors_host(res, case.key, res, case.key, pairs)


# ------------------------------------------------------------------ graph -> KV
def test_graph_then_kv(gpu):
    """The pass reads nothing but an order plane: the same call behind the graph executor."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    path = os.path.join(golden, "synth_n5_mix.npz")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    import make_golden as G
    with np.load(path) as z:
        planes = fs.synth_host(fs.synth_params(**G.params_from_array(z["params"])))
    S, steps, keys = min(planes.S, 65), planes.steps, 7
    batch = fd.run_batch(planes, metrics=False)
    rng = np.random.RandomState(5)
    key = rng.randint(0, keys, planes.plane).astype(np.uint32)
    kinds = rng.choice([K.GET, K.PUT, K.PUT, K.DELETE], planes.plane).astype(np.uint32)
    ops = (kinds << 30) | np.where(kinds == K.PUT, rng.randint(1, 1 << 30, planes.plane), 0).astype(np.uint32)
    res = fd.run_kv(batch.order, batch.nexec, key, ops, planes.S, steps, keys, 1, fill=0xA5,
                    before_launch=poisoner(*FILLS[2]))
    same_bytes(res, K.run_kv_host(batch.order, batch.nexec, key, ops, planes.S, steps, keys, 1, fill=0xA5))
    assert np.all(batch.err == 0) and int(batch.nexec.sum()) > 0 and np.any(batch.order & 0x80000000)
    for s in range(S):
        rows = _lib.index(np.arange(steps), s, steps)
        order = [int(x) & 0x7FFFFFFF for x in batch.order[_lib.index(np.arange(int(batch.nexec[s])), s, steps)]]
        kv_ref.check_stream(res, s, order, [int(k) for k in key[rows]], [[int(o)] for o in ops[rows]])


# ------------------------------------------------------------------ op generator
def test_op_generator_equals_its_host_twin(gpu):
    S, steps = 65, 37
    lengths = np.array([(11 * s) % (steps + 1) for s in range(S)], np.uint32)
    for fill, L in zip(FILLS, (lengths, None, lengths)):
        dev = fd.synth_kv_ops(21, S, steps, 35, 15, lengths=L, stream_base=1 << 31, before_launch=poisoner(*fill))
        host = K.synth_kv_ops_host(21, S, steps, 35, 15, L, stream_base=1 << 31)
        assert np.array_equal(dev.download(np.uint32, _lib.plane_words(S, steps)), host)
