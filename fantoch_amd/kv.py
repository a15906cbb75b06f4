"""The KV stage (fx_kv_execute and friends): op words, op planes, the result
object, and the host twins.  The device calls are in fantoch_amd.device
(run_kv, compare_monitors, synth_kv_ops).  Either side: KvSession, the stage
fed in pieces behind an executor session (fx_kv_advance, fx_kv_session_monitor
and their host twins).

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


SESSION_NAMES = ("result", "store", "rank", "err")


class KvSessionResult:
    """Outputs of a KvSession as host arrays: result (omax planes by arrival
    row, cumulative), store [S, keys], rank (plane by arrival row), err [S]."""

    def __init__(self, S, steps, keys, omax, result, store, rank, err):
        self.S, self.steps, self.keys, self.omax = S, steps, keys, omax
        self.plane = _lib.plane_words(S, steps)
        self.result, self.rank, self.err, self.status = result, rank, err, 0
        self.store = store.reshape(S, keys)

    results = KvResult.results


class KvSession:
    """The KV stage fed in pieces (fx_kv_advance, or fx_kv_advance_host with
    host=True), behind an executor session: owns the state and the four
    outputs of S streams of up to `steps` rows for its lifetime; all five start
    as the byte `fill` (None: as allocated on the device, zero on the host).
    The planes handed to advance() are the whole streams' planes every time;
    nexec says how far each stream's order plane has come and does not
    decrease from call to call."""

    def __init__(self, S, steps, keys, omax=1, fill=None, host=False):
        lib = _lib.load()
        self.S, self.steps, self.keys, self.omax, self.host = int(S), int(steps), int(keys), int(omax), bool(host)
        self.fill = fill
        self.plane = pw = _lib.plane_words(self.S, self.steps)
        self.state_bytes = lib.fx_kv_session_bytes(self.keys, self.S)
        self.started = False
        self._keep, self._last = [], None
        sizes = (max(self.omax, 1) * pw, self.S * self.keys, pw, self.S)
        if self.host:
            word = np.uint32((fill or 0) * 0x01010101)
            self.out = {name: np.full(n, word, np.uint32) for name, n in zip(SESSION_NAMES, sizes)}
            self.state = np.full(self.state_bytes, fill or 0, np.uint8)
        else:
            from . import device as fd
            self.out = {name: fd.DeviceBuffer(n * 4) for name, n in zip(SESSION_NAMES, sizes)}
            self.state = fd.DeviceBuffer(self.state_bytes)
            if fill is not None:
                for b in list(self.out.values()) + [self.state]:
                    b.fill_bytes(fill)

    @property
    def dev(self):
        """The device buffers of the outputs by name (None on the host)."""
        return None if self.host else dict(self.out)

    def fill_outputs(self, fill, names=SESSION_NAMES):
        """The outputs `names` filled with the byte `fill` again (the state stays)."""
        for name in names:
            if self.host:
                self.out[name][:] = np.uint32(fill * 0x01010101)
            else:
                self.out[name].fill_bytes(fill)

    def state_words(self):
        """A host copy of the state as it is now."""
        if self.host:
            return self.state.view(np.uint32).copy()
        return self.state.download(np.uint32, self.state_bytes // 4)

    def _ptr(self, x):
        return x.ctypes.data if self.host else x.ptr

    def _batch(self, order, nexec, key, ops, key_mask, steps=None, keys=None, omax=None):
        if self.host:
            arrs = [_u32(x) for x in (order, nexec, key, ops)]
            keep = arrs
        else:
            from . import device as fd
            keep = []
            arrs = [fd._dev(x, keep) for x in (order, nexec, key, ops)]
            keep = keep + arrs
        inb = _lib.KvBatch(self._ptr(arrs[0]), self._ptr(arrs[1]), self._ptr(arrs[2]), key_mask, self._ptr(arrs[3]),
                           self.S, self.steps if steps is None else int(steps),
                           self.keys if keys is None else int(keys), self.omax if omax is None else int(omax))
        return inb, keep

    def launch(self, order, nexec, key, ops, key_mask=0xFFFFFFFF, init=None, before_launch=None, **contract):
        """One fx_kv_advance (asynchronous on the device).  order / nexec / key
        / ops: host arrays on the host; host arrays or DeviceBuffers on the
        device.  init None: the session's first call passes FX_FLAG_INIT.
        contract (steps, keys, omax): values other than the session's (a call
        that breaks the contract).  A refused call raises."""
        lib = _lib.load()
        init = (not self.started) if init is None else bool(init)
        flags = _lib.FX_FLAG_INIT if init else 0
        inb, keep = self._batch(order, nexec, key, ops, key_mask, **contract)
        self._keep = keep  # alive until the next launch
        if not contract:
            self._last = (inb, keep)
        outb = _lib.KvSessionOut(*[self._ptr(self.out[name]) for name in SESSION_NAMES])
        if self.host:
            check(lib.fx_kv_advance_host(ctypes.byref(inb), ctypes.byref(outb), self.state.ctypes.data, flags),
                  "fx_kv_advance_host")
        else:
            if before_launch is not None:
                before_launch(None)
            check(lib.fx_kv_advance(ctypes.byref(inb), ctypes.byref(outb), self.state.ptr, flags, None),
                  "fx_kv_advance")
        self.started = True

    def _download(self, name):
        if self.host:
            return self.out[name].copy()
        return self.out[name].download(np.uint32, self.out[name].nbytes // 4)

    def result(self):
        """Host copies of the cumulative outputs as they are now (a KvSessionResult)."""
        if not self.host:
            check(_lib.load().fx_dev_synchronize(None), "sync")
        return KvSessionResult(self.S, self.steps, self.keys, self.omax, *[self._download(n) for n in SESSION_NAMES])

    def advance(self, order, nexec, key, ops, key_mask=0xFFFFFFFF, init=None, before_launch=None, **contract):
        """launch(), then the cumulative outputs after the call."""
        self.launch(order, nexec, key, ops, key_mask, init, before_launch, **contract)
        return self.result()

    def monitor(self, fill=None, before_launch=None):
        """fx_kv_session_monitor over the planes of the last advance(): the
        monitor of the rows consumed so far.  monitor, mon_off, store and err
        start as the byte `fill` (None: the session's, or 0).  Returns a
        KvResult whose result planes are the session's."""
        lib = _lib.load()
        if self._last is None:
            raise ValueError("KvSession.monitor: no call yet")
        inb = self._last[0]
        fill = (self.fill or 0) if fill is None else fill
        sizes = dict(store=self.S * self.keys, monitor=self.plane, mon_off=self.S * (self.keys + 1), err=self.S)
        if self.host:
            word = np.uint32(fill * 0x01010101)
            out = {name: np.full(n, word, np.uint32) for name, n in sizes.items()}
            outb = _lib.KvOut(self.out["result"].ctypes.data, out["store"].ctypes.data, out["monitor"].ctypes.data,
                              out["mon_off"].ctypes.data, out["err"].ctypes.data)
            check(lib.fx_kv_session_monitor_host(ctypes.byref(inb), self.out["rank"].ctypes.data, ctypes.byref(outb),
                                                 self.state.ctypes.data), "fx_kv_session_monitor_host")
            host = out
        else:
            from . import device as fd
            out = {name: fd.DeviceBuffer(n * 4) for name, n in sizes.items()}
            for b in out.values():
                b.fill_bytes(fill)
            outb = _lib.KvOut(self.out["result"].ptr, out["store"].ptr, out["monitor"].ptr, out["mon_off"].ptr,
                              out["err"].ptr)
            if before_launch is not None:
                before_launch(None)
            check(lib.fx_kv_session_monitor(ctypes.byref(inb), self.out["rank"].ptr, ctypes.byref(outb),
                                            self.state.ptr, None), "fx_kv_session_monitor")
            check(lib.fx_dev_synchronize(None), "sync")
            host = {name: b.download(np.uint32, b.nbytes // 4) for name, b in out.items()}
        return KvResult(self.S, self.steps, self.keys, self.omax, self._download("result"), host["store"],
                        host["monitor"], host["mon_off"], host["err"], 0, None if self.host else out)


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
