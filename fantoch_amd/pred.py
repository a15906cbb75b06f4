"""The predecessors executor (Caesar) fed in pieces: PredSession over
fx_pred_advance (device) or fx_pred_advance_host (host=True), and
run_pred_host, the host twin as a one-call session.  Whole streams on the
device: fantoch_amd.device.run_pred.

A batch is what run_pred takes: the stream planes (fantoch_amd.streams.Planes:
dot, hdr, deps, S, steps, dmax, n), the two Caesar clock planes and, optionally,
the ndeps plane.  The outputs are an executor's: order, release, nexec, err.

Batches in the shape of Caesar's own commits (every conflicting command of a
lower timestamp as a dep, clocks moved by retries; the model is
csrc/fx_pred_synth.h): pred_synth_params, pred_synth_shape, pred_synth_host and
pred_synth_device."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check

SMALL, LDS, HBM = _lib.FX_PRED_TIER_SMALL, _lib.FX_PRED_TIER_LDS, _lib.FX_PRED_TIER_HBM
NAMES = ("order", "release", "nexec", "err")
INPUTS = ("dot", "hdr", "deps", "clock_lo", "clock_hi", "ndeps")


class PredResult:
    """order and release (planes), nexec / err [S] as host arrays; `dev`: the
    device buffers by the same names (a device session)."""

    def __init__(self, S, steps, order, release, nexec, err, status=0, dev=None):
        self.S, self.steps, self.plane = S, steps, _lib.plane_words(S, steps)
        self.order, self.release, self.nexec, self.err = order, release, nexec, err
        self.status, self.dev = status, dev

    def executed(self, s, k0=0):
        """Arrival rows of stream s in execution order, from order row k0 on."""
        rows = self.order[_lib.index(np.arange(k0, int(self.nexec[s])), s, self.steps)]
        return [int(x) & 0x7FFFFFFF for x in rows]


def _u32(a):
    return np.ascontiguousarray(a, np.uint32)


def _flags(execute_at_commit):
    return _lib.FX_FLAG_EXECUTE_AT_COMMIT if execute_at_commit else 0


def _filled(S, steps, fill):
    pw = _lib.plane_words(S, steps)
    word = np.uint32(fill * 0x01010101)
    return {name: np.full(n, word, np.uint32) for name, n in zip(NAMES, (pw, pw, S, S))}


class PredSession:
    """S streams of up to `steps` rows at one table tier, fed in pieces: owns
    the state and the four outputs for its lifetime; all five start as the byte
    `fill` (None: as allocated on the device, zero on the host).  The planes
    handed to launch() are the whole streams' planes every time; lengths say how
    far each stream has come and do not decrease from call to call."""

    def __init__(self, S, steps, n, dmax, tier, execute_at_commit=False, fill=None, host=False):
        lib = _lib.load()
        self.S, self.steps, self.n, self.dmax, self.tier = int(S), int(steps), int(n), int(dmax), int(tier)
        self.at_commit, self.host = bool(execute_at_commit), bool(host)
        self.plane = pw = _lib.plane_words(self.S, self.steps)
        self.state_bytes = lib.fx_pred_session_bytes(self.tier, self.n, self.dmax, self.S)
        if self.state_bytes == 0 and self.S:
            raise _lib.FxError(_lib.FX_ERR_UNSUPPORTED, "fx_pred_session_bytes: the tier's tables do not fit")
        self.started = False
        self._keep, self._inputs = [], None
        self._committed = np.zeros(self.S, np.int64)   # rows handed over at the last committed_and_executed()
        self._executed = np.zeros(self.S, np.int64)    # nexec then
        self._dot = None
        if self.host:
            self.out = _filled(self.S, self.steps, fill or 0)
            self.state = np.full(max(self.state_bytes, 16), fill or 0, np.uint8)
        else:
            from . import device as fd
            self.out = {name: fd.DeviceBuffer(k * 4) for name, k in zip(NAMES, (pw, pw, self.S, self.S))}
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
            return self.state[:self.state_bytes].view(np.uint32).copy()
        return self.state.download(np.uint32, self.state_bytes // 4)

    def _batch(self, planes, clock_lo, clock_hi, ndeps):
        """The six input planes where the call reads them (uploaded once per
        distinct `planes` object on the device)."""
        key = (id(planes), id(clock_lo), id(clock_hi), id(ndeps))
        if self._inputs is not None and self._inputs[0] == key:
            return self._inputs[1]
        arrs = dict(dot=planes.dot, hdr=planes.hdr, deps=planes.deps, clock_lo=clock_lo, clock_hi=clock_hi, ndeps=ndeps)
        if self.host:
            bufs = {k: (None if v is None else _u32(v)) for k, v in arrs.items()}
            ptrs = {k: (None if v is None else v.ctypes.data) for k, v in bufs.items()}
        else:
            from . import device as fd
            keep = []
            bufs = {k: (None if v is None else fd._dev(v, keep)) for k, v in arrs.items()}
            bufs["_keep"] = keep
            ptrs = {k: (None if bufs[k] is None else bufs[k].ptr) for k in INPUTS}
        self._inputs = (key, (bufs, ptrs), (planes, clock_lo, clock_hi, ndeps))
        self._dot = planes.dot
        return self._inputs[1]

    def launch(self, planes, clock_lo, clock_hi, ndeps, lengths, init=None, before_launch=None, steps=None,
               execute_at_commit=None, tier=None, dmax=None, drop_ndeps=False):
        """One fx_pred_advance (asynchronous on the device) over the batch and
        `lengths` (None: every stream has `steps` rows): host arrays on the
        host; host arrays or DeviceBuffers on the device.  init None: the
        session's first call passes FX_FLAG_INIT.  steps, execute_at_commit,
        tier, dmax, drop_ndeps: values other than the session's (a call that
        breaks the contract).  A refused call raises."""
        lib = _lib.load()
        init = (not self.started) if init is None else bool(init)
        at_commit = self.at_commit if execute_at_commit is None else bool(execute_at_commit)
        flags = (_lib.FX_FLAG_INIT if init else 0) | _flags(at_commit)
        steps = self.steps if steps is None else int(steps)
        tier = self.tier if tier is None else int(tier)
        dmax = self.dmax if dmax is None else int(dmax)
        _, ptrs = self._batch(planes, clock_lo, clock_hi, ndeps)
        if self.host:
            lengths = None if lengths is None else _u32(lengths)
            self._keep = [lengths]
            lptr = lengths.ctypes.data if lengths is not None else None
        else:
            from . import device as fd
            keep = []
            lengths = None if lengths is None else fd._dev(lengths, keep)
            self._keep = keep  # alive until the next launch
            lptr = lengths.ptr if lengths else None
        base = _lib.StreamBatch(ptrs["dot"], ptrs["hdr"], ptrs["deps"], lptr, self.S, steps, dmax, self.n)
        inb = _lib.PredBatch(base, ptrs["clock_lo"], ptrs["clock_hi"], None if drop_ndeps else ptrs["ndeps"])
        if self.host:
            outb = _lib.OrderBatch(*[self.out[name].ctypes.data for name in NAMES])
            check(lib.fx_pred_advance_host(ctypes.byref(inb), ctypes.byref(outb), tier, self.state.ctypes.data, flags),
                  "fx_pred_advance_host")
        else:
            outb = _lib.OrderBatch(*[self.out[name].ptr for name in NAMES])
            if before_launch is not None:
                before_launch(None)
            check(lib.fx_pred_advance(ctypes.byref(inb), ctypes.byref(outb), tier, self.state.ptr, flags, None),
                  "fx_pred_advance")
        if init:
            self._committed[:] = 0
            self._executed[:] = 0
        self.started = True

    def result(self):
        """Host copies of the cumulative outputs as they are now (a PredResult)."""
        if self.host:
            return PredResult(self.S, self.steps, *[self.out[name].copy() for name in NAMES])
        check(_lib.load().fx_dev_synchronize(None), "sync")
        return PredResult(self.S, self.steps,
                          *[self.out[name].download(np.uint32, self.out[name].nbytes // 4) for name in NAMES],
                          dev=self.dev)

    def advance(self, planes, clock_lo, clock_hi, ndeps, lengths, init=None, before_launch=None, **contract):
        """launch(), then the cumulative outputs after the call."""
        self.launch(planes, clock_lo, clock_hi, ndeps, lengths, init, before_launch, **contract)
        return self.result()

    def committed_and_executed(self, lengths, result=None):
        """Executor::executed's answer per stream (pred/mod.rs:92-97): (dots
        newly committed, the dots newly executed) since the previous call of
        this method.  lengths: the rows handed over so far (host values, None:
        `steps` each); committed counts rows, a stopped stream's unhandled ones
        included; executed is order rows [nexec then, nexec now) through the dot
        plane (host dot planes only).  result: a result() taken after the last
        launch, else one is taken."""
        res = self.result() if result is None else result
        lens = np.full(self.S, self.steps, np.int64) if lengths is None else \
            np.minimum(np.asarray(lengths, np.int64), self.steps)
        lens = np.maximum(lens, self._committed)
        dot = np.asarray(self._dot, np.uint32)
        out = []
        for s in range(self.S):
            k0, k1 = int(self._executed[s]), int(res.nexec[s])
            rows = res.order[_lib.index(np.arange(k0, k1), s, self.steps)] & np.uint32(0x7FFFFFFF)
            dots = dot[_lib.index(rows.astype(np.int64), s, self.steps)]
            out.append((int(lens[s] - self._committed[s]), [(int(d) >> 24, int(d) & 0xFFFFFF) for d in dots]))
            self._executed[s] = k1
        self._committed = lens
        return out


def run_pred_host(planes, clock_lo, clock_hi, ndeps, tier, execute_at_commit=False, fill=0):
    """The host twin over a whole batch: a one-call session.  Every output
    starts filled with the byte `fill`.  Returns a PredResult."""
    ses = PredSession(planes.S, planes.steps, planes.n, planes.dmax, tier, execute_at_commit, fill=fill, host=True)
    return ses.advance(planes, clock_lo, clock_hi, ndeps, planes.lengths)


def pred_synth_params(seed=1, instances=1, n=5, cmds=100, window=8, horizon=4, max_bump=2, retry_pct=30,
                      conflicts=(2, 10, 50, 100), instance_base=0, conflict_block=0):
    """fx_pred_synth_params: dmax = n (horizon + max_bump + 1) - 1."""
    p = _lib.PredSynthParams()
    p.seed, p.instances, p.instance_base, p.n, p.cmds_per_process = seed, instances, instance_base, n, cmds
    p.window, p.horizon, p.max_bump, p.retry_pct = window, horizon, max_bump, retry_pct
    p.num_conflicts = len(conflicts)
    for i, c in enumerate(conflicts):
        p.conflict_pct[i] = c
    p.conflict_block = conflict_block
    return p


def pred_synth_shape(params):
    """(S, steps, dmax) of a parameter set; a refused one raises."""
    S, steps, dmax = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    check(_lib.load().fx_pred_synth_shape(ctypes.byref(params), ctypes.byref(S), ctypes.byref(steps),
                                          ctypes.byref(dmax)), "fx_pred_synth_shape")
    return S.value, steps.value, dmax.value


def pred_synth_host(params, fill=0, ndeps=True):
    """The streams generated on the host (the same bytes as the device's):
    (planes, clock_lo, clock_hi, ndeps), as tests/pred_shapes.pack_pred_streams
    returns them.  Every buffer starts as the byte `fill` (the generator leaves
    pad rows and pad streams alone); ndeps=False: no ndeps plane (dmax <= 31),
    None in its place."""
    from . import streams as fs
    S, steps, dmax = pred_synth_shape(params)
    pw = _lib.plane_words(S, steps)
    word = np.uint32(fill * 0x01010101)
    dot, hdr, clo, chi = (np.full(pw, word, np.uint32) for _ in range(4))
    deps = np.full(max(dmax, 1) * pw, word, np.uint32)
    nd = np.full(pw, word, np.uint32) if ndeps else None
    pl = _lib.PredSynthPlanes(dot.ctypes.data, hdr.ctypes.data, deps.ctypes.data, clo.ctypes.data, chi.ctypes.data,
                              nd.ctypes.data if ndeps else None)
    check(_lib.load().fx_pred_synth_generate_host(ctypes.byref(params), ctypes.byref(pl)),
          "fx_pred_synth_generate_host")
    return fs.Planes(S, steps, dmax, params.n, dot=dot, hdr=hdr, deps=deps), clo, chi, nd


def pred_synth_device(params, dev, fill=0, ndeps=True, form=None):
    """The streams generated on the device `dev` (a torch device), on the
    current stream: int32 tensors (dot, hdr, deps, clock_lo, clock_hi, ndeps)
    whose data_ptr()s are ready for _lib.StreamBatch / _lib.PredBatch.  fill,
    ndeps: as pred_synth_host; form: a named form of the kernel
    (_lib.FX_PRED_SYNTH_FORM_*, measurement), None: the library's."""
    import torch
    S, steps, dmax = pred_synth_shape(params)
    pw = _lib.plane_words(S, steps)
    word = int(np.uint32(fill * 0x01010101).view(np.int32))

    def buf(words):
        return torch.full((words,), word, dtype=torch.int32, device=dev)
    dot, hdr, clo, chi = buf(pw), buf(pw), buf(pw), buf(pw)
    deps = buf(max(dmax, 1) * pw)
    nd = buf(pw) if ndeps else None
    pl = _lib.PredSynthPlanes(dot.data_ptr(), hdr.data_ptr(), deps.data_ptr(), clo.data_ptr(), chi.data_ptr(),
                              nd.data_ptr() if ndeps else None)
    hs = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib = _lib.load()
    if form is None:
        check(lib.fx_pred_synth_generate(ctypes.byref(params), ctypes.byref(pl), hs), "fx_pred_synth_generate")
    else:
        check(lib.fx_pred_synth_generate_form(ctypes.byref(params), ctypes.byref(pl), int(form), hs),
              "fx_pred_synth_generate_form")
    return dot, hdr, deps, clo, chi, nd
