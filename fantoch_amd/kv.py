"""The KV stage (fx_kv_execute and friends): op words, op planes, the result
object, and the host twins.  The device calls are in fantoch_amd.device
(run_kv, compare_monitors, synth_kv_ops).

Canonical C15: a value is an id in 1 .. 2^30 - 1, 0 is None.  A partial is a
list of op words on one key; `ops` planes are indexed by arrival row, slot j
of a partial in plane j."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check

GET, PUT, DELETE, EMPTY = _lib.FX_KV_GET, _lib.FX_KV_PUT, _lib.FX_KV_DELETE, _lib.FX_KV_EMPTY
VALUE_MASK = (1 << 30) - 1


def kv_op(kind, value=0):
    """FX_KV_OP(kind, value)."""
    return ((int(kind) & 3) << 30) | (int(value) & VALUE_MASK)


def op_kind(op):
    return int(op) >> 30


def op_value(op):
    return int(op) & VALUE_MASK


def pack_kv_ops(streams, steps, omax=None):
    """streams[s][a] = the op words of arrival row a of stream s (a list of up
    to FX_KV_MAX_OPS words; rows past the list are empty partials).  Returns
    (planes, omax): omax planes of plane_words(S, steps) words, unused slots
    FX_KV_OP(FX_KV_EMPTY, 0)."""
    S = len(streams)
    if omax is None:
        omax = max([len(p) for rows in streams for p in rows] + [1])
    if not 1 <= omax <= _lib.FX_KV_MAX_OPS:
        raise ValueError("pack_kv_ops: omax outside 1..FX_KV_MAX_OPS")
    pw = _lib.plane_words(S, steps)
    planes = np.full(omax * pw, kv_op(EMPTY), np.uint32)
    for s, rows in enumerate(streams):
        if len(rows) > steps:
            raise ValueError("pack_kv_ops: stream %d has more rows than steps" % s)
        for a, partial in enumerate(rows):
            if len(partial) > omax:
                raise ValueError("pack_kv_ops: a partial with more than omax ops")
            at = int(_lib.index(a, s, steps))
            for j, op in enumerate(partial):
                planes[j * pw + at] = op
    return planes, omax


class KvResult:
    """Outputs of fx_kv_execute as host arrays: result (omax planes by arrival
    row), store [S, keys], monitor (plane), mon_off [S, keys + 1], err [S] and
    the call's status.  `dev` (run_kv(keep_device=True)): the device buffers by
    the same names."""

    def __init__(self, S, steps, keys, omax, result, store, monitor, mon_off, err, status, dev=None):
        self.S, self.steps, self.keys, self.omax = S, steps, keys, omax
        self.plane = _lib.plane_words(S, steps)
        self.result, self.monitor, self.err, self.status, self.dev = result, monitor, err, status, dev
        self.store = store.reshape(S, keys)
        self.mon_off = mon_off.reshape(S, keys + 1)

    def results(self, s, a):
        """The omax result words of arrival row a of stream s."""
        at = int(_lib.index(a, s, self.steps))
        return [int(self.result[j * self.plane + at]) for j in range(self.omax)]


def monitor_rows(result, s, k):
    """Arrival rows of the write partials executed on key k of stream s, in
    execution order (ExecutionOrderMonitor::get_order of the key, as rows)."""
    lo, hi = int(result.mon_off[s, k]), int(result.mon_off[s, k + 1])
    return [int(x) for x in result.monitor[_lib.index(np.arange(lo, hi), s, result.steps)]]


def _u32(a):
    return np.ascontiguousarray(a, np.uint32)


def run_kv_host(order, nexec, key, ops, S, steps, keys, omax, key_mask=0xFFFFFFFF, fill=0):
    """fx_kv_execute_host over host arrays; every output starts filled with the
    byte `fill`.  Returns a KvResult (a refused call: its status, outputs as filled)."""
    order, nexec, key, ops = _u32(order), _u32(nexec), _u32(key), _u32(ops)
    pw = _lib.plane_words(S, steps)
    word = np.uint32(fill * 0x01010101)
    result, monitor = np.full(max(omax, 1) * pw, word, np.uint32), np.full(pw, word, np.uint32)
    store, mon_off, err = np.full(S * keys, word, np.uint32), np.full(S * (keys + 1), word, np.uint32), \
        np.full(S, word, np.uint32)
    inb = _lib.KvBatch(order.ctypes.data, nexec.ctypes.data, key.ctypes.data, key_mask, ops.ctypes.data, S, steps, keys,
                       omax)
    outb = _lib.KvOut(result.ctypes.data, store.ctypes.data, monitor.ctypes.data, mon_off.ctypes.data, err.ctypes.data)
    status = _lib.load().fx_kv_execute_host(ctypes.byref(inb), ctypes.byref(outb))
    return KvResult(S, steps, keys, omax, result, store, monitor, mon_off, err, status)


def compare_monitors_host(a, rifl_a, b, rifl_b, pairs):
    """fx_kv_monitor_compare_host: a, b KvResults, rifl_* the planes that name
    the commands by arrival row, pairs [(stream of a, stream of b)].  Returns
    [(key, position)] per pair, (FX_KV_AGREE, FX_KV_AGREE) where they agree."""
    rifl_a, rifl_b = _u32(rifl_a), _u32(rifl_b)
    pairs = _u32(np.asarray(pairs, np.uint32).reshape(-1, 2))
    diff = np.zeros(pairs.shape, np.uint32)
    mo = [_u32(x.mon_off) for x in (a, b)]
    ma = _lib.KvMonitor(a.monitor.ctypes.data, mo[0].ctypes.data, rifl_a.ctypes.data, a.S, a.steps, a.keys)
    mb = _lib.KvMonitor(b.monitor.ctypes.data, mo[1].ctypes.data, rifl_b.ctypes.data, b.S, b.steps, b.keys)
    check(_lib.load().fx_kv_monitor_compare_host(ctypes.byref(ma), ctypes.byref(mb), pairs.ctypes.data, len(pairs),
                                                 diff.ctypes.data), "fx_kv_monitor_compare_host")
    return [(int(k), int(p)) for k, p in diff]


def synth_kv_ops_host(seed, S, steps, read_pct=0, delete_pct=0, lengths=None, stream_base=0):
    """fx_kv_synth_ops_host: one op plane of plane_words(S, steps) words."""
    ops = np.zeros(_lib.plane_words(S, steps), np.uint32)
    lengths = None if lengths is None else _u32(lengths)
    check(_lib.load().fx_kv_synth_ops_host(seed, stream_base, read_pct, delete_pct,
                                           lengths.ctypes.data if lengths is not None else None, S, steps,
                                           ops.ctypes.data), "fx_kv_synth_ops_host")
    return ops
