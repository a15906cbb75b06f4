"""The pending stage (fx_pending_aggregate and friends): AggregatePending for
the batched engines.  A command's partials, one order row per (rifl, key), are
collected per rifl; a command is named by its head row (the arrival row of its
first executed partial) and is ready when its last partial has executed.  The
device calls are in fantoch_amd.device (run_pending).  Either side:
PendingSession, the stage fed in pieces behind an executor session
(fx_pending_advance and its host twin).

Canonical C16: the partials of a command are listed in execution order."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check

MAX_PARTS, IGNORED = _lib.FX_PENDING_MAX_PARTS, _lib.FX_PENDING_IGNORED
ONCHIP, HBM = _lib.FX_PENDING_TIER_ONCHIP, _lib.FX_PENDING_TIER_HBM
NAMES = ("part", "head", "ready", "index", "nready", "nopen", "err")


class PendingResult:
    """Outputs of the pending stage as host arrays: part (MAX_PARTS planes by
    head row), head (plane by arrival row), ready (plane), index (plane by head
    row), nready / nopen / err [S], the call's status and the streams rerun on
    the HBM tier.  `dev` (run_pending(keep_device=True)): the device buffers by
    the same names."""

    def __init__(self, S, steps, part, head, ready, index, nready, nopen, err, status, reruns=0, dev=None):
        self.S, self.steps, self.plane = S, steps, _lib.plane_words(S, steps)
        self.part, self.head, self.ready, self.index = part, head, ready, index
        self.nready, self.nopen, self.err, self.status, self.reruns, self.dev = nready, nopen, err, status, reruns, dev
        # the rifl and count planes the call read with its count_mask and process (host copies):
        # command_results names a command and counts its partials with them
        self.rifl = self.count = None
        self.count_mask, self.process = 0xFFFFFFFF, 0

    def members(self, s, head):
        """The partials of the command with head row `head`: the count the stage read at that row."""
        at = int(_lib.index(head, s, self.steps))
        if self.process and int(self.rifl[at]) >> 24 != self.process:
            return 0
        return int(self.count[at]) & self.count_mask

    def ready_heads(self, s):
        """Head rows of the completed commands of stream s, in completion order."""
        return [int(h) for h in self.ready[_lib.index(np.arange(int(self.nready[s])), s, self.steps)]]

    def parts(self, s, head, count):
        """Arrival rows of the first `count` partials of the command with head row `head`."""
        at = int(_lib.index(head, s, self.steps))
        return [int(self.part[j * self.plane + at]) for j in range(count)]


def _u32(a):
    return np.ascontiguousarray(a, np.uint32)


def run_pending_host(order, nexec, rifl, count, S, steps, count_mask=0xFFFFFFFF, process=0, tier=HBM, fill=0):
    """fx_pending_aggregate_host over host arrays; every output starts filled
    with the byte `fill`.  Returns a PendingResult (a refused call: its status,
    outputs as filled)."""
    order, nexec, rifl, count = _u32(order), _u32(nexec), _u32(rifl), _u32(count)
    pw = _lib.plane_words(S, steps)
    word = np.uint32(fill * 0x01010101)
    out = {name: np.full(n, word, np.uint32)
           for name, n in zip(NAMES, (MAX_PARTS * pw, pw, pw, pw, S, S, S))}
    inb = _lib.PendingBatch(order.ctypes.data, nexec.ctypes.data, rifl.ctypes.data, count.ctypes.data, count_mask,
                            process, S, steps)
    outb = _lib.PendingOut(*[out[name].ctypes.data for name in NAMES])
    status = _lib.load().fx_pending_aggregate_host(ctypes.byref(inb), ctypes.byref(outb), tier)
    res = PendingResult(S, steps, *[out[name] for name in NAMES], status)
    res.rifl, res.count, res.count_mask, res.process = rifl, count, count_mask, process
    return res


class PendingSession:
    """The pending stage fed in pieces (fx_pending_advance, or
    fx_pending_advance_host with host=True), behind an executor session: owns
    the state and the seven outputs of S streams of up to `steps` rows for its
    lifetime; all start as the byte `fill` (None: as allocated on the device,
    zero on the host).  count_mask and process are the session's.  The planes
    handed to advance() are the whole streams' planes every time; nexec does
    not decrease from call to call."""

    def __init__(self, S, steps, count_mask=0xFFFFFFFF, process=0, fill=None, host=False):
        lib = _lib.load()
        self.S, self.steps, self.host = int(S), int(steps), bool(host)
        self.count_mask, self.process = int(count_mask), int(process)
        self.plane = pw = _lib.plane_words(self.S, self.steps)
        self.state_bytes = lib.fx_pending_session_bytes(self.steps, self.S)
        self.started = False
        self._keep, self._planes, self._fresh, self._res = [], None, False, None
        self._nready = [np.zeros(self.S, np.uint32), np.zeros(self.S, np.uint32)]  # before / after the last call
        sizes = (MAX_PARTS * pw, pw, pw, pw, self.S, self.S, self.S)
        if self.host:
            word = np.uint32((fill or 0) * 0x01010101)
            self.out = {name: np.full(n, word, np.uint32) for name, n in zip(NAMES, sizes)}
            self.state = np.full(self.state_bytes, fill or 0, np.uint8)
        else:
            from . import device as fd
            self.out = {name: fd.DeviceBuffer(n * 4) for name, n in zip(NAMES, sizes)}
            self.state = fd.DeviceBuffer(self.state_bytes)
            if fill is not None:
                for b in list(self.out.values()) + [self.state]:
                    b.fill_bytes(fill)

    @property
    def dev(self):
        """The device buffers of the outputs by name (None on the host)."""
        return None if self.host else dict(self.out)

    def fill_outputs(self, fill, names=NAMES):
        """The outputs `names` filled with the byte `fill` again (the state stays)."""
        for name in names:
            if self.host:
                self.out[name][:] = np.uint32(fill * 0x01010101)
            else:
                self.out[name].fill_bytes(fill)

    def state_words(self):
        """A host copy of the state as it is now (opaque, and each side's own)."""
        if self.host:
            return self.state.view(np.uint32).copy()
        return self.state.download(np.uint32, self.state_bytes // 4)

    def launch(self, order, nexec, rifl, count, init=None, before_launch=None, steps=None, count_mask=None,
               process=None):
        """One fx_pending_advance (asynchronous on the device).  order / nexec
        / rifl / count: host arrays on the host; host arrays or DeviceBuffers
        on the device.  init None: the session's first call passes
        FX_FLAG_INIT.  steps, count_mask, process: values other than the
        session's (a call that breaks the contract).  A refused call raises."""
        lib = _lib.load()
        init = (not self.started) if init is None else bool(init)
        flags = _lib.FX_FLAG_INIT if init else 0
        steps = self.steps if steps is None else int(steps)
        count_mask = self.count_mask if count_mask is None else int(count_mask)
        process = self.process if process is None else int(process)
        if self.host:
            arrs = [_u32(x) for x in (order, nexec, rifl, count)]
            self._keep = arrs
            ptrs = [x.ctypes.data for x in arrs]
        else:
            from . import device as fd
            keep = []
            arrs = [fd._dev(x, keep) for x in (order, nexec, rifl, count)]
            self._keep = keep + arrs  # alive until the next launch
            ptrs = [x.ptr for x in arrs]
        self._planes = (arrs[2], arrs[3])
        inb = _lib.PendingBatch(*ptrs, count_mask, process, self.S, steps)
        if self.host:
            outb = _lib.PendingOut(*[self.out[name].ctypes.data for name in NAMES])
            check(lib.fx_pending_advance_host(ctypes.byref(inb), ctypes.byref(outb), self.state.ctypes.data, flags),
                  "fx_pending_advance_host")
        else:
            outb = _lib.PendingOut(*[self.out[name].ptr for name in NAMES])
            if before_launch is not None:
                before_launch(None)
            check(lib.fx_pending_advance(ctypes.byref(inb), ctypes.byref(outb), self.state.ptr, flags, None),
                  "fx_pending_advance")
        self.started = True
        self._fresh = True

    def result(self):
        """Host copies of the cumulative outputs as they are now (a
        PendingResult that command_results reads as any other)."""
        pw = self.plane
        if self.host:
            res = PendingResult(self.S, self.steps, *[self.out[name].copy() for name in NAMES], 0)
            if self._planes is not None:
                res.rifl, res.count = self._planes[0].copy(), self._planes[1].copy()
        else:
            check(_lib.load().fx_dev_synchronize(None), "sync")
            res = PendingResult(self.S, self.steps,
                                *[self.out[name].download(np.uint32, self.out[name].nbytes // 4) for name in NAMES], 0,
                                dev=self.dev)
            if self._planes is not None:
                res.rifl, res.count = (p.download(np.uint32, pw) for p in self._planes)
        res.count_mask, res.process = self.count_mask, self.process
        if self._fresh:  # the first look after a call: the window of new_ready moves
            self._fresh = False
            if self.started:
                self._nready = [self._nready[1], res.nready.copy()]
        self._res = res
        return res

    def advance(self, order, nexec, rifl, count, init=None, before_launch=None, **contract):
        """launch(), then the cumulative outputs after the call."""
        if init or not self.started:
            self._nready = [np.zeros(self.S, np.uint32), np.zeros(self.S, np.uint32)]
        self.launch(order, nexec, rifl, count, init, before_launch, **contract)
        return self.result()

    def new_ready(self, s):
        """Head rows of the commands of stream s that the last call completed,
        in completion order: the `ready` rows between the nready before that
        call and the nready after it."""
        if self._fresh:
            self.result()
        lo, hi = int(self._nready[0][s]), int(self._nready[1][s])
        if not lo <= hi <= self.steps:  # counts that no call of the session wrote
            return []
        return [int(h) for h in self._res.ready[_lib.index(np.arange(lo, hi), s, self.steps)]]


def command_results(pending, kv, key_plane, s, key_mask=0xFFFFFFFF, ops=None):
    """The CommandResults of stream s, in completion order: [(rifl, {key:
    [results]})], a result None or the value's id.  pending: a PendingResult;
    kv: the KvResult of the same order plane; key_plane: the key plane the KV
    stage read.  A command's rifl and the number of its partials are the rifl
    and the count the pending stage read at its head row (a completed command
    has exactly that many), so nothing here depends on what the outputs held
    before the call.  ops (the op planes): a partial's results stop at its
    first unused slot; without them every partial has kv.omax."""
    steps, rifl = pending.steps, pending.rifl
    out = []
    for h in pending.ready_heads(s):
        per_key = {}
        for a in pending.parts(s, h, pending.members(s, h)):
            at = int(_lib.index(a, s, steps))
            res = kv.results(s, a)
            if ops is not None:
                res = [r for j, r in enumerate(res) if int(ops[j * pending.plane + at]) >> 30 != _lib.FX_KV_EMPTY]
            per_key[int(key_plane[at]) & key_mask] = [r or None for r in res]
        out.append((int(rifl[int(_lib.index(h, s, steps))]), per_key))
    return out
