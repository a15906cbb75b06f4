"""The slot executor (fx_slot_execute and friends): FPaxos's SlotExecutor for a
batch.  A stream is a list of slot numbers by arrival row (slots are 1-based);
the input is one plane of them.  The outputs are an executor's: order, release,
nexec, err, which the KV stage and the pending stage read as they are.

Host side: pack_slot_streams, run_slot_host, synth_slot_host and the
generator's restatement synth_slot_streams_c6.  Device side: run_slot,
synth_slot.  Either side: SlotSession, streams fed in pieces
(fx_slot_advance, fx_slot_advance_host).

Canonical C6: the generator's draw is the counter RNG of the other generators,
keyed by (seed, global stream, slot, purpose 17)."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check

LANE, SCAN = _lib.FX_SLOT_TIER_LANE, _lib.FX_SLOT_TIER_SCAN
LANE_WINDOW = _lib.FX_SLOT_LANE_WINDOW
NAMES = ("order", "release", "nexec", "err")
SLOT_DRAW = 17
_M64 = (1 << 64) - 1


class SlotResult:
    """Outputs of the slot executor as host arrays: order and release (planes),
    nexec / err [S], the call's status and the streams rerun on the SCAN tier
    (run_slot(lane_first=True)).
    `dev` (run_slot(keep_device=True)): the device buffers by the same names,
    and the slot plane as "slot"."""

    def __init__(self, S, steps, order, release, nexec, err, status, reruns=0, dev=None):
        self.S, self.steps, self.plane = S, steps, _lib.plane_words(S, steps)
        self.order, self.release, self.nexec, self.err = order, release, nexec, err
        self.status, self.reruns, self.dev = status, reruns, dev

    def executed(self, s):
        """Arrival rows of stream s in execution order."""
        rows = self.order[_lib.index(np.arange(int(self.nexec[s])), s, self.steps)]
        return [int(x) & 0x7FFFFFFF for x in rows]

    def released(self, s, rows):
        """release of the first `rows` arrival rows of stream s."""
        return [int(x) for x in self.release[_lib.index(np.arange(rows), s, self.steps)]]


def _u32(a):
    return np.ascontiguousarray(a, np.uint32)


def pack_slot_streams(streams, steps=None):
    """streams[s] = the slots of stream s by arrival row.  Returns (plane,
    lengths, S, steps): the plane of plane_words(S, steps) words (0 where a
    stream has no row) and the streams' lengths."""
    S = len(streams)
    if steps is None:
        steps = max([len(x) for x in streams] + [1])
    plane = np.zeros(_lib.plane_words(S, steps), np.uint32)
    for s, rows in enumerate(streams):
        if len(rows) > steps:
            raise ValueError("pack_slot_streams: stream %d has more rows than steps" % s)
        if len(rows):
            plane[_lib.index(np.arange(len(rows)), s, steps)] = np.asarray(rows, np.uint32)
    return plane, np.array([len(x) for x in streams], np.uint32), S, steps


def unpack_slot_streams(plane, lengths, S, steps):
    """The inverse of pack_slot_streams (lengths None: every stream has `steps` rows)."""
    return [[int(x) for x in plane[_lib.index(np.arange(steps if lengths is None else int(lengths[s])), s, steps)]]
            for s in range(S)]


def _flags(execute_at_commit):
    return _lib.FX_FLAG_EXECUTE_AT_COMMIT if execute_at_commit else 0


def _filled(S, steps, fill):
    pw = _lib.plane_words(S, steps)
    word = np.uint32(fill * 0x01010101)
    return {name: np.full(n, word, np.uint32) for name, n in zip(NAMES, (pw, pw, S, S))}


def run_slot_host(plane, lengths, S, steps, execute_at_commit=False, fill=0):
    """fx_slot_execute_host over host arrays; every output starts filled with
    the byte `fill`.  Returns a SlotResult (a refused call: its status, outputs
    as filled)."""
    plane = _u32(plane)
    lengths = None if lengths is None else _u32(lengths)
    out = _filled(S, steps, fill)
    inb = _lib.SlotBatch(plane.ctypes.data, lengths.ctypes.data if lengths is not None else None, S, steps)
    outb = _lib.OrderBatch(*[out[name].ctypes.data for name in NAMES])
    status = _lib.load().fx_slot_execute_host(ctypes.byref(inb), ctypes.byref(outb), _flags(execute_at_commit))
    return SlotResult(S, steps, *[out[name] for name in NAMES], status)


def _mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def slot_draw(seed, g, s):
    """The generator's draw for slot s of global stream g (synth_rand of fx_synth.h, purpose 17)."""
    return _mix64((_mix64((_mix64(seed ^ 0x5851F42D4C957F2D) + g) & _M64) + (s << 8) + SLOT_DRAW) & _M64)


def synth_slot_streams_c6(seed, S, steps, window, lengths=None, stream_base=0):
    """The generator restated in Python: per stream the slots 1 .. L sorted by
    (slot + draw % window, slot).  Returns the streams as lists of slots."""
    if window < 1:
        raise ValueError("synth_slot_streams_c6: window must be at least 1")
    streams = []
    for s in range(S):
        L = steps if lengths is None else min(int(lengths[s]), steps)
        g = stream_base + s
        streams.append(sorted(range(1, L + 1), key=lambda k: (k + slot_draw(seed, g, k) % window, k)))
    return streams


def synth_slot_host(seed, S, steps, window, lengths=None, stream_base=0, fill=0):
    """fx_slot_synth_generate_host: the slot plane (every word of it is
    written; it starts as the byte `fill`)."""
    plane = np.full(_lib.plane_words(S, steps), np.uint32(fill * 0x01010101), np.uint32)
    lengths = None if lengths is None else _u32(lengths)
    check(_lib.load().fx_slot_synth_generate_host(seed, stream_base, S, steps,
                                                  lengths.ctypes.data if lengths is not None else None, window,
                                                  plane.ctypes.data), "fx_slot_synth_generate_host")
    return plane


# ------------------------------------------------------------------ device
def synth_slot(seed, S, steps, window, lengths=None, stream_base=0, fill=None, before_launch=None):
    """fx_slot_synth_generate: the slot plane generated on the device (lengths:
    None, a host array or a DeviceBuffer; fill: the byte the plane holds before
    the launch).  Returns the DeviceBuffer."""
    from . import device as fd
    keep = []
    plane = fd.DeviceBuffer(_lib.plane_words(S, steps) * 4)
    if fill is not None:
        plane.fill_bytes(fill)
    lengths = None if lengths is None else fd._dev(lengths, keep)
    if before_launch is not None:
        before_launch(None)
    check(_lib.load().fx_slot_synth_generate(seed, stream_base, S, steps, lengths.ptr if lengths else None, window,
                                             plane.ptr, None), "fx_slot_synth_generate")
    check(_lib.load().fx_dev_synchronize(None), "sync")
    return plane


def run_slot(plane, lengths, S, steps, execute_at_commit=False, tier=None, fill=0, stream_map=None,
             before_launch=None, keep_device=False, lane_first=False):
    """The slot executor over a batch: fx_slot_run (tier None: every stream at
    SCAN, or with lane_first at LANE and then at SCAN the streams that left the
    lane window) or one fx_slot_execute at `tier` (stream_map: the streams of
    the launch, None = all).  plane / lengths: host
    arrays or DeviceBuffers.  Every output, and the SCAN tier's state, starts
    filled with the byte `fill`.  before_launch(stream): called right before
    the first launch.  Returns a SlotResult; a refused call raises, a stream's
    status lands in err."""
    from . import device as fd
    lib = _lib.load()
    keep = []
    plane = fd._dev(plane, keep)
    lengths = None if lengths is None else fd._dev(lengths, keep)
    pw = _lib.plane_words(S, steps)
    out = {name: fd.DeviceBuffer(n * 4) for name, n in zip(NAMES, (pw, pw, S, S))}
    for b in out.values():
        b.fill_bytes(fill)
    inb = _lib.SlotBatch(plane.ptr, lengths.ptr if lengths else None, S, steps)
    outb = _lib.OrderBatch(*[out[name].ptr for name in NAMES])
    flags = _flags(execute_at_commit)
    reruns = ctypes.c_uint32()
    if tier is not None:
        lanes, dmap, state = S, None, None
        if stream_map is not None:
            lanes, dmap = len(stream_map), fd._dev(stream_map, keep)
        if tier == SCAN:
            state = fd.DeviceBuffer(lib.fx_slot_state_bytes(steps, lanes))
            state.fill_bytes(fill)
        if before_launch is not None:
            before_launch(None)
        check(lib.fx_slot_execute(ctypes.byref(inb), ctypes.byref(outb), dmap.ptr if dmap else None, lanes, tier,
                                  state.ptr if state else None, flags, None), "fx_slot_execute")
        check(lib.fx_dev_synchronize(None), "sync")
    else:
        if before_launch is not None:
            before_launch(None)
        if lane_first:
            flags |= _lib.first_tier_flag(LANE)
        check(lib.fx_slot_run(ctypes.byref(inb), ctypes.byref(outb), flags, None, ctypes.byref(reruns)), "fx_slot_run")
    return SlotResult(S, steps, *[out[name].download(np.uint32, out[name].nbytes // 4) for name in NAMES], 0,
                      int(reruns.value), dict(out, slot=plane) if keep_device else None)


class SlotSession:
    """The slot executor fed in pieces (fx_slot_advance, or fx_slot_advance_host
    with host=True): owns the state and the four outputs of S streams of up to
    `steps` rows for its lifetime; all five start as the byte `fill` (None: as
    allocated on the device, zero on the host).  The plane handed to advance()
    is the whole stream's plane every time; lengths say how far each stream
    has come and do not decrease from call to call."""

    def __init__(self, S, steps, execute_at_commit=False, fill=None, host=False):
        lib = _lib.load()
        self.S, self.steps, self.at_commit, self.host = int(S), int(steps), bool(execute_at_commit), bool(host)
        self.plane = pw = _lib.plane_words(self.S, self.steps)
        self.state_bytes = lib.fx_slot_session_bytes(self.steps, self.S)
        self.started = False
        self._keep = []
        if self.host:
            self.out = _filled(self.S, self.steps, fill or 0)
            self.state = np.full(self.state_bytes, fill or 0, np.uint8)
        else:
            from . import device as fd
            self.out = {name: fd.DeviceBuffer(n * 4) for name, n in zip(NAMES, (pw, pw, self.S, self.S))}
            self.state = fd.DeviceBuffer(self.state_bytes)
            if fill is not None:
                for b in list(self.out.values()) + [self.state]:
                    b.fill_bytes(fill)

    @property
    def dev(self):
        """The device buffers of the outputs by name (None on the host): what
        run_kv / run_pending read the cumulative order plane from."""
        return None if self.host else dict(self.out)

    def fill_outputs(self, fill, names=NAMES):
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

    def launch(self, plane, lengths, init=None, before_launch=None, steps=None, execute_at_commit=None):
        """One fx_slot_advance (asynchronous on the device) over plane /
        lengths: host arrays on the host; host arrays or DeviceBuffers on the
        device (lengths None: every stream has `steps` rows).  init None: the
        session's first call passes FX_FLAG_INIT.  steps, execute_at_commit:
        values other than the session's (a call that breaks the contract).
        A refused call raises."""
        lib = _lib.load()
        init = (not self.started) if init is None else bool(init)
        at_commit = self.at_commit if execute_at_commit is None else bool(execute_at_commit)
        flags = (_lib.FX_FLAG_INIT if init else 0) | _flags(at_commit)
        steps = self.steps if steps is None else int(steps)
        if self.host:
            plane = _u32(plane)
            lengths = None if lengths is None else _u32(lengths)
            self._keep = [plane, lengths]
            inb = _lib.SlotBatch(plane.ctypes.data, lengths.ctypes.data if lengths is not None else None, self.S, steps)
            outb = _lib.OrderBatch(*[self.out[name].ctypes.data for name in NAMES])
            check(lib.fx_slot_advance_host(ctypes.byref(inb), ctypes.byref(outb), self.state.ctypes.data, flags),
                  "fx_slot_advance_host")
        else:
            from . import device as fd
            keep = []
            plane = fd._dev(plane, keep)
            lengths = None if lengths is None else fd._dev(lengths, keep)
            self._keep = keep  # alive until the next launch
            inb = _lib.SlotBatch(plane.ptr, lengths.ptr if lengths else None, self.S, steps)
            outb = _lib.OrderBatch(*[self.out[name].ptr for name in NAMES])
            if before_launch is not None:
                before_launch(None)
            check(lib.fx_slot_advance(ctypes.byref(inb), ctypes.byref(outb), self.state.ptr, flags, None),
                  "fx_slot_advance")
        self.started = True

    def result(self):
        """Host copies of the cumulative outputs as they are now (a SlotResult)."""
        if self.host:
            return SlotResult(self.S, self.steps, *[self.out[name].copy() for name in NAMES], 0)
        check(_lib.load().fx_dev_synchronize(None), "sync")
        return SlotResult(self.S, self.steps,
                          *[self.out[name].download(np.uint32, self.out[name].nbytes // 4) for name in NAMES], 0,
                          dev=self.dev)

    def advance(self, plane, lengths, init=None, before_launch=None, **contract):
        """launch(), then the cumulative outputs after the call."""
        self.launch(plane, lengths, init, before_launch, **contract)
        return self.result()
