"""Device-side batch execution through the C-ABI (fx_dev_* plumbing, no torch needed).

`run_batch(planes)` uploads a host `Planes` batch, runs the GPU executor
(fx_batch_run_tiered: tier 0 for every stream, capacity reruns at tiers 1/2)
and the metrics pass, and returns host copies of the outputs.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check


class DeviceBuffer:
    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        check(_lib.load().fx_dev_alloc(ctypes.byref(p), max(self.nbytes, 16)), "fx_dev_alloc")
        self.ptr = p.value

    def upload(self, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        if arr.nbytes:
            check(_lib.load().fx_dev_h2d(self.ptr, arr.ctypes.data, arr.nbytes, stream), "fx_dev_h2d")

    def upload_at(self, offset, arr, stream=None):
        """Uploads arr to the buffer from byte `offset` on."""
        arr = np.ascontiguousarray(arr)
        assert 0 <= offset and offset + arr.nbytes <= self.nbytes
        check(_lib.load().fx_dev_h2d(self.ptr + int(offset), arr.ctypes.data, arr.nbytes, stream), "fx_dev_h2d")

    def download(self, dtype, count, stream=None):
        out = np.empty(count, dtype)
        check(_lib.load().fx_dev_d2h(out.ctypes.data, self.ptr, out.nbytes, stream), "fx_dev_d2h")
        check(_lib.load().fx_dev_synchronize(stream), "fx_dev_synchronize")
        return out

    def zero(self, stream=None):
        check(_lib.load().fx_dev_memset(self.ptr, 0, self.nbytes, stream), "fx_dev_memset")

    def fill_bytes(self, value, stream=None):
        check(_lib.load().fx_dev_memset(self.ptr, value, self.nbytes, stream), "fx_dev_memset")

    def free(self):
        if self.ptr:
            _lib.load().fx_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_count():
    return _lib.load().fx_device_count()


class BatchResult:
    def __init__(self, order, release, nexec, err, chain, delay, tier_counts, status, cut_stats=None):
        self.order = order
        self.release = release
        self.nexec = nexec
        self.err = err
        self.chain = chain
        self.delay = delay
        self.tier_counts = tier_counts
        self.status = status
        self.cut_stats = cut_stats


def _upload(named, lengths, S):
    """The named host arrays on the device, and the streams' lengths (None: none)."""
    bufs = {}
    for name, arr in named:
        arr = np.ascontiguousarray(arr)
        bufs[name] = DeviceBuffer(arr.nbytes)
        bufs[name].upload(arr)
    dl = None
    if lengths is not None:
        dl = DeviceBuffer(S * 4)
        dl.upload(np.asarray(lengths, np.uint32))
    return bufs, dl


def _order_outputs(S, pw, order_fill=None):
    """The order outputs of a launch and the OrderBatch over them: order (filled with the byte
    order_fill, None: as allocated), release (FX_RELEASE_NONE: rows a stream never reaches stay
    so), nexec and err (0xAB: every driver writes every stream's count and status, the sentinel
    shows any it skipped)."""
    order, release, nexec, err = DeviceBuffer(pw * 4), DeviceBuffer(pw * 4), DeviceBuffer(S * 4), DeviceBuffer(S * 4)
    if order_fill is not None:
        order.fill_bytes(order_fill)
    release.fill_bytes(0xFF)
    nexec.fill_bytes(0xAB)
    err.fill_bytes(0xAB)
    return order, release, nexec, err, _lib.OrderBatch(order.ptr, release.ptr, nexec.ptr, err.ptr)


def run_metrics(hdr, order, release, nexec, S, steps, nbins_chain, nbins_delay, chain0=None, delay0=None):
    """fx_batch_metrics over the planes hdr, order and release and the counts
    nexec of S streams of `steps` rows (host arrays or DeviceBuffers); dot,
    deps and lengths are passed as null.  The histograms are device buffers of
    exactly nbins words and one guard word (fantoch_amd.metrics.GUARD) behind
    them; the bins start at chain0 / delay0 (None: zero).  Returns (chain,
    delay) as downloaded, each with its guard word as the last element; a
    refused call raises."""
    from . import metrics
    keep = []
    hdr, order, release, nexec = (_dev(x, keep) for x in (hdr, order, release, nexec))
    hists = []
    for nbins, start in ((nbins_chain, chain0), (nbins_delay, delay0)):
        host = metrics.guarded(nbins, start)
        hists.append(DeviceBuffer(host.nbytes))
        hists[-1].upload(host)
    inb = _lib.StreamBatch(None, hdr.ptr, None, None, S, steps, 0, 0)
    outb = _lib.OrderBatch(order.ptr, release.ptr, nexec.ptr, None)
    hb = _lib.HistBatch(hists[0].ptr, nbins_chain, hists[1].ptr, nbins_delay)
    check(_lib.load().fx_batch_metrics(ctypes.byref(inb), ctypes.byref(outb), ctypes.byref(hb), None),
          "fx_batch_metrics")
    return hists[0].download(np.uint64, nbins_chain + 1), hists[1].download(np.uint64, nbins_delay + 1)


def run_batch(planes, execute_at_commit=False, nbins_chain=64, nbins_delay=4096, tiered=True,
              tier=None, init_frontier=None, metrics=True, cut=False, before_launch=None, order_fill=None,
              stream_map=None):
    """Runs a host batch on the GPU; returns host outputs (BatchResult).

    cut: fx_batch_run_cut (quiescent-cut decomposition, for huge streams);
    tiered: fx_batch_run_tiered starting at `tier` (None = FX_TIER_DEFAULT);
    otherwise one fx_batch_execute launch at `tier` (None = FX_TIER_DEFAULT).
    before_launch(stream): called with the launch's stream (None = the null
    stream) once the inputs are on the device, right before the first
    executor launch (tests: register poisoning, tests/test_poison_all.py).
    order_fill: the byte order, release, nexec, err and a tier's state hold
    before the launch (None: as _order_outputs leaves them, the state as
    allocated).  stream_map (single launch only): lane l of the launch runs
    stream stream_map[l], the other streams are not touched, and no histogram
    is taken (chain and delay None)."""
    if stream_map is not None and (cut or (tiered and init_frontier is None)):
        raise ValueError("run_batch: only the single launch takes a stream_map")
    lib = _lib.load()
    S, steps, pw = planes.S, planes.steps, planes.plane
    bufs, lengths = _upload((("dot", planes.dot), ("hdr", planes.hdr), ("deps", planes.deps)), planes.lengths, S)
    order, release, nexec, err, outb = _order_outputs(S, pw)
    if order_fill is not None:
        for b in (order, release, nexec, err):
            b.fill_bytes(order_fill)
    lanes, dmap = S, None
    if stream_map is not None:
        lanes = len(stream_map)
        dmap = DeviceBuffer(lanes * 4)
        dmap.upload(np.asarray(stream_map, np.uint32))
    inb = _lib.StreamBatch(bufs["dot"].ptr, bufs["hdr"].ptr, bufs["deps"].ptr,
                           lengths.ptr if lengths else None, S, steps, planes.dmax, planes.n)
    flags = _lib.FX_FLAG_EXECUTE_AT_COMMIT if execute_at_commit else 0
    tier_counts = (ctypes.c_uint32 * _lib.FX_NUM_TIERS)()
    cut_stats = None
    if before_launch is not None:
        before_launch(None)
    if cut:
        cut_stats = _lib.CutStats()
        status = lib.fx_batch_run_cut(ctypes.byref(inb), ctypes.byref(outb), flags, None,
                                      ctypes.byref(cut_stats))
    elif tiered and init_frontier is None:
        tflags = flags | (_lib.first_tier_flag(tier) if tier is not None else 0)
        status = lib.fx_batch_run_tiered(ctypes.byref(inb), ctypes.byref(outb), tflags, None, tier_counts)
    else:
        tier = _lib.FX_TIER_DEFAULT if tier is None else tier
        front = None
        if init_frontier is not None:
            front = DeviceBuffer(S * 8 * 4)
            front.upload(np.asarray(init_frontier, np.uint32).reshape(S, 8))
        state = None
        if tier in (_lib.FX_TIER_GLOBAL, _lib.FX_TIER_SPLIT, _lib.FX_TIER_WIDE_HBM):  # HBM-resident tier's working memory / split scratch
            state = DeviceBuffer(lib.fx_batch_state_bytes(tier, planes.n, lanes))
            if order_fill is not None:
                state.fill_bytes(order_fill)
        status = lib.fx_batch_execute(ctypes.byref(inb), ctypes.byref(outb), tier, dmap.ptr if dmap else None, lanes,
                                      state.ptr if state else None, 0, steps,
                                      flags | _lib.FX_FLAG_INIT, front.ptr if front else None, None)
        check(status, "fx_batch_execute")
        check(lib.fx_dev_synchronize(None), "sync")
        tier_counts[tier] = lanes
    chain = delay = None
    if metrics and not execute_at_commit and stream_map is None:
        chain, delay = (h[:-1] for h in run_metrics(bufs["hdr"], order, release, nexec, S, steps, nbins_chain,
                                                    nbins_delay))
    res = BatchResult(order.download(np.uint32, pw), release.download(np.uint32, pw),
                      nexec.download(np.uint32, S), err.download(np.uint32, S),
                      chain, delay, list(tier_counts), status, cut_stats)
    return res


def run_pred(planes, clock_lo, clock_hi, ndeps=None, execute_at_commit=False, tier=None, nbins_delay=4096,
             before_launch=None, stream_map=None, fill=None):
    """PredecessorsExecutor over a host batch with packed Caesar clock planes:
    fx_pred_run (tier None: the escalation chain) or one fx_pred_execute at
    `tier` (FX_PRED_TIER_*); returns a BatchResult (delay histogram from
    fx_batch_metrics).  stream_map (with a tier): lane l of the launch runs
    stream stream_map[l], the other streams are not touched, and no histogram
    is taken (delay None).  fill: the byte order, release, nexec, err and the
    HBM tier's state hold before the launch (None: as _order_outputs leaves
    them, the state as allocated)."""
    if stream_map is not None and tier is None:
        raise ValueError("run_pred: fx_pred_run takes no stream_map")
    lib = _lib.load()
    S, steps, pw = planes.S, planes.steps, planes.plane
    bufs, lengths = _upload((("dot", planes.dot), ("hdr", planes.hdr), ("deps", planes.deps),
                             ("clo", np.asarray(clock_lo, np.uint32)), ("chi", np.asarray(clock_hi, np.uint32)),
                             ("nd", np.asarray(ndeps if ndeps is not None else [0], np.uint32))), planes.lengths, S)
    order, release, nexec, err, outb = _order_outputs(S, pw)
    if fill is not None:
        for b in (order, release, nexec, err):
            b.fill_bytes(fill)
    lanes, dmap = S, None
    if stream_map is not None:
        lanes = len(stream_map)
        dmap = DeviceBuffer(lanes * 4)
        dmap.upload(np.asarray(stream_map, np.uint32))
    base = _lib.StreamBatch(bufs["dot"].ptr, bufs["hdr"].ptr, bufs["deps"].ptr, lengths.ptr if lengths else None,
                            S, steps, planes.dmax, planes.n)
    inb = _lib.PredBatch(base, bufs["clo"].ptr, bufs["chi"].ptr, bufs["nd"].ptr if ndeps is not None else None)
    flags = _lib.FX_FLAG_EXECUTE_AT_COMMIT if execute_at_commit else 0
    reruns = ctypes.c_uint32()
    if before_launch is not None:
        before_launch(None)
    if tier is not None:
        state = DeviceBuffer(lib.fx_pred_state_bytes(planes.n, planes.dmax, lanes)) if tier == _lib.FX_PRED_TIER_HBM \
            else None
        if state is not None and fill is not None:
            state.fill_bytes(fill)
        status = lib.fx_pred_execute(ctypes.byref(inb), ctypes.byref(outb), dmap.ptr if dmap else None, lanes, tier,
                                     state.ptr if state else None, flags, None)
        check(lib.fx_dev_synchronize(None), "sync")
    else:
        status = lib.fx_pred_run(ctypes.byref(inb), ctypes.byref(outb), flags, None, ctypes.byref(reruns))
    chain = delay = None
    if stream_map is None:  # the histograms go over every stream's nexec
        chain, delay = (h[:-1] for h in run_metrics(bufs["hdr"], order, release, nexec, S, steps, 64, nbins_delay))
    res = BatchResult(order.download(np.uint32, pw), release.download(np.uint32, pw), nexec.download(np.uint32, S),
                      err.download(np.uint32, S), chain, delay, [], status)
    res.reruns = int(reruns.value)
    return res


class TableResult:
    def __init__(self, order, release, nexec, err, stable_clock, reruns, status, stable_sent=None, dev=None):
        self.dev = dev  # run_table(keep_device=True): the device buffers order / release / nexec / err
        self.order = order
        self.release = release
        self.nexec = nexec
        self.err = err
        self.stable_clock = stable_clock
        self.reruns = reruns
        self.status = status
        self.stable_sent = stable_sent


def _tile_download(lengths, S, plane, steps, tile):
    """(streams, lengths, part) of plane tile `tile` of S streams of `steps`
    rows in device memory: part(buf, nplanes) copies the tile's words of each
    of buf's planes to the host (asynchronously: synchronise before use)."""
    lib = _lib.load()
    S = min(64, S - 64 * tile)
    tw = _lib.plane_words(64, steps)
    host = np.empty(S, np.uint32)
    check(lib.fx_dev_d2h(host.ctypes.data, lengths.ptr + 256 * tile, S * 4, None), "fx_dev_d2h")

    def part(buf, nplanes=1):
        out = np.empty(nplanes * tw, np.uint32)
        for j in range(nplanes):
            check(lib.fx_dev_d2h(out.ctypes.data + j * tw * 4, buf.ptr + (j * plane + tile * tw) * 4, tw * 4, None),
                  "fx_dev_d2h")
        return out

    return S, host, part


class DeviceTable:
    """The planes of an fx_table_batch_mk in device memory, filled by
    fx_table_synth_generate: S = params.streams streams of up to `steps` rows
    (None: the longest stream, found by the counting pass; at least 1), vmax =
    fast_quorum vote slots, an nkeys plane when params.kmax > 1.  generate()
    fills the planes; run_table takes the object as it takes TablePlanes, with
    no upload; download() gives the host copy."""
    ps = False

    def __init__(self, params, steps=None):
        lib = _lib.load()
        self.params = params
        self.S, self.n, self.keys, self.vmax = int(params.streams), int(params.n), int(params.keys), \
            int(params.fast_quorum)
        nbytes = lib.fx_table_synth_scratch_bytes(ctypes.byref(params))
        if nbytes == 0:
            raise _lib.FxError(_lib.FX_ERR_INVALID_ARG, "fx_table_synth_scratch_bytes")
        self.scratch = DeviceBuffer(nbytes)
        self.lengths = DeviceBuffer(self.S * 4)
        self.longest = None
        if steps is None:
            steps = max(self.count(), 1)
        self.steps = int(steps)
        self.plane = pw = _lib.plane_words(self.S, self.steps)
        self.bufs = {name: DeviceBuffer(pw * 4) for name in ("hdr", "dot", "clock")}
        self.bufs["votes"] = DeviceBuffer(3 * self.vmax * pw * 4)
        self.bufs["nkeys"] = DeviceBuffer(pw * 4) if params.kmax > 1 else None

    @property
    def nkeys(self):
        return self.bufs["nkeys"]

    def count(self):
        """fx_table_synth_lengths: the longest stream (the lengths stay on the device)."""
        longest = ctypes.c_uint32()
        check(_lib.load().fx_table_synth_lengths(ctypes.byref(self.params), self.lengths.ptr, self.scratch.ptr, None,
                                                 ctypes.byref(longest)), "fx_table_synth_lengths")
        self.longest = longest.value
        return self.longest

    def fill_bytes(self, value):
        """Every plane and the lengths filled with one byte (tests: what a call leaves untouched)."""
        for b in list(self.bufs.values()) + [self.lengths]:
            if b is not None:
                b.fill_bytes(value)

    def generate(self):
        """fx_table_synth_generate into the planes; returns the status."""
        planes = _lib.TableSynthPlanes(self.bufs["hdr"].ptr, self.bufs["dot"].ptr, self.bufs["clock"].ptr,
                                       self.bufs["votes"].ptr, self.nkeys.ptr if self.nkeys else None,
                                       self.lengths.ptr)
        return _lib.load().fx_table_synth_generate(ctypes.byref(self.params), ctypes.byref(planes), self.steps,
                                                   self.scratch.ptr, None)

    def download(self):
        """The planes as fantoch_amd.table.TablePlanes."""
        from . import table
        p = table.TablePlanes(self.S, self.steps, self.n, self.keys, self.vmax,
                              lengths=self.lengths.download(np.uint32, self.S))
        p.hdr, p.dot, p.clock = (self.bufs[name].download(np.uint32, self.plane) for name in ("hdr", "dot", "clock"))
        p.votes = self.bufs["votes"].download(np.uint32, 3 * self.vmax * self.plane)
        if self.nkeys is not None:
            p.nkeys = self.nkeys.download(np.uint32, self.plane)
        return p

    def download_tile(self, tile):
        """The 64 streams of plane tile `tile` as TablePlanes (stream s of the
        launch is stream s % 64 of tile s // 64)."""
        from . import table
        S, lengths, part = _tile_download(self.lengths, self.S, self.plane, self.steps, tile)
        p = table.TablePlanes(S, self.steps, self.n, self.keys, self.vmax, lengths=lengths)
        p.hdr, p.dot, p.clock, p.votes = part(self.bufs["hdr"]), part(self.bufs["dot"]), part(self.bufs["clock"]), \
            part(self.bufs["votes"], 3 * self.vmax)
        if self.nkeys is not None:
            p.nkeys = part(self.nkeys)
        check(_lib.load().fx_dev_synchronize(None), "fx_dev_synchronize")
        return p


def synth_table(params, steps=None, before_launch=None):
    """Tempo-shaped vote streams generated on the device
    (fx_table_synth_generate; fantoch_amd.table.table_synth_params): returns
    the DeviceTable holding them.  before_launch(stream): called right before
    the generator's first launch (tests: register poisoning)."""
    t = DeviceTable(params, steps)
    if before_launch is not None:
        before_launch(None)
    check(t.generate(), "fx_table_synth_generate")
    return t


def run_table(planes, stability_threshold, execute_at_commit=False, tier=None, order_fill=0, multi=None,
              shards=None, keep_device=False):
    """Tempo's TableExecutor over a host batch (fantoch_amd.table.TablePlanes)
    or over streams generated on the device (DeviceTable: no upload):
    fx_table_run (tier None: ONCHIP, then HBM for the streams that ran out of
    capacity) or one fx_table_execute at `tier` (FX_TABLE_TIER_*); the _mk
    entry points (multi-key commands) when the batch has an nkeys plane, or
    when `multi` is true (a missing plane then counts as all ones); the _ps
    entry points (StableAtShard events, commands that span shards) when the
    planes are marked `ps`, or when `shards` is true (nkeys words without a
    shard count then count as one shard).  Returns a TableResult: order /
    release planes, nexec, err, stable_clock [S, keys], reruns, the status and,
    from the _ps entry points, the stable_sent plane (None otherwise).  The
    order plane starts filled with the byte order_fill, the release and
    stable_sent planes with FX_RELEASE_NONE.  keep_device: the result's `dev`
    holds the device buffers of order / release / nexec / err (and the input
    planes by name), so a later stage (run_kv) reads them where they are."""
    lib = _lib.load()
    S, pw = planes.S, planes.plane
    on_device = isinstance(planes, DeviceTable)
    if on_device:
        if shards:
            raise ValueError("run_table: streams generated on the device have no shard counts")
        bufs, lengths = planes.bufs, planes.lengths
    else:
        bufs, lengths = _upload([(name, getattr(planes, name)) for name in ("hdr", "dot", "clock", "votes")],
                                planes.lengths, S)
    order, release, nexec, err, outb = _order_outputs(S, pw, order_fill)
    stable = DeviceBuffer(S * planes.keys * 4)
    stable.fill_bytes(0xAB)
    inb = _lib.TableBatch(bufs["hdr"].ptr, bufs["dot"].ptr, bufs["clock"].ptr, bufs["votes"].ptr,
                          lengths.ptr if lengths else None, S, planes.steps, planes.n, planes.keys, planes.vmax,
                          int(stability_threshold))
    flags = _lib.FX_FLAG_EXECUTE_AT_COMMIT if execute_at_commit else 0
    reruns = ctypes.c_uint32()
    ps = bool(getattr(planes, "ps", False))
    if shards is None:
        shards = ps
    if shards and multi is False:
        raise ValueError("run_table: shards needs the multi-key entry points")
    if ps and not shards:
        raise ValueError("run_table: the planes hold StableAtShard events or shard counts")
    if multi is None:
        multi = planes.nkeys is not None
    execute, run, state_bytes = lib.fx_table_execute, lib.fx_table_run, lib.fx_table_state_bytes
    sent = None
    if multi and on_device and planes.nkeys is not None:
        inb = _lib.TableBatchMk(inb, planes.nkeys.ptr)
        execute, run = lib.fx_table_execute_mk, lib.fx_table_run_mk
    elif multi or shards:
        nkeys_h = planes.nkeys if planes.nkeys is not None else np.full(pw, 0x101 if ps else 1, np.uint32)
        nkeys_h = np.ascontiguousarray(nkeys_h, np.uint32)
        if shards and not ps:  # plain nkeys words: one shard each (a word that is no nkeys stays invalid)
            nkeys_h = np.where(nkeys_h < 256, nkeys_h | np.uint32(1 << 8), np.uint32(0)).astype(np.uint32)
        nkeys = DeviceBuffer(pw * 4)
        nkeys.upload(nkeys_h)
        inb = _lib.TableBatchMk(inb, nkeys.ptr)
        execute, run = lib.fx_table_execute_mk, lib.fx_table_run_mk
    if shards:
        sent = DeviceBuffer(pw * 4)
        sent.fill_bytes(0xFF)
        state_bytes = lib.fx_table_state_bytes_ps
        execute = lambda i, o, st, *rest: lib.fx_table_execute_ps(i, o, st, sent.ptr, *rest)
        run = lambda i, o, st, *rest: lib.fx_table_run_ps(i, o, st, sent.ptr, *rest)
    if tier is not None:
        state = DeviceBuffer(state_bytes(planes.n, planes.keys, S)) if tier == _lib.FX_TABLE_TIER_HBM else None
        check(execute(ctypes.byref(inb), ctypes.byref(outb), stable.ptr, None, S, tier,
                      state.ptr if state else None, flags, None), "fx_table_execute")
        check(lib.fx_dev_synchronize(None), "sync")
        status = 0
    else:
        status = run(ctypes.byref(inb), ctypes.byref(outb), stable.ptr, flags, None, ctypes.byref(reruns))
        # the call itself failed (a stream's status lands in err; FX_ERR_INVALID_ARG can be either: a
        # call that was refused has written no stream's status)
        if status in (_lib.FX_ERR_NO_DEVICE, _lib.FX_ERR_HIP, _lib.FX_ERR_UNSUPPORTED) or \
                (status == _lib.FX_ERR_INVALID_ARG and np.all(err.download(np.uint32, S) == 0xABABABAB)):
            check(status, "fx_table_run")
    return TableResult(order.download(np.uint32, pw), release.download(np.uint32, pw), nexec.download(np.uint32, S),
                       err.download(np.uint32, S), stable.download(np.uint32, S * planes.keys).reshape(S, planes.keys),
                       int(reruns.value), status, sent.download(np.uint32, pw) if sent is not None else None,
                       dict(bufs, order=order, release=release, nexec=nexec, err=err) if keep_device else None)


def _dev(x, keep):
    """x on the device: a DeviceBuffer as it is, a host array uploaded (and kept alive in `keep`)."""
    if isinstance(x, DeviceBuffer):
        return x
    arr = np.ascontiguousarray(x, np.uint32)
    b = DeviceBuffer(arr.nbytes)
    b.upload(arr)
    keep.append(b)
    return b


def run_kv(order, nexec, key, ops, S, steps, keys, omax=1, key_mask=0xFFFFFFFF, fill=0, before_launch=None,
           keep_device=False):
    """fx_kv_execute: KVStore results, final stores and per-key monitors of a
    batch, from the order plane an executor wrote.  order / nexec / key / ops:
    host arrays or DeviceBuffers (the outputs of run_table(keep_device=True)
    and the planes of a DeviceTable are used where they are).  Every output
    starts filled with the byte `fill`.  before_launch(stream): called right
    before the launch (tests: register poisoning).  Returns a
    fantoch_amd.kv.KvResult; a refused call raises."""
    from . import kv
    lib = _lib.load()
    keep = []
    order, nexec, key, ops = (_dev(x, keep) for x in (order, nexec, key, ops))
    pw = _lib.plane_words(S, steps)
    out = {"result": DeviceBuffer(max(omax, 1) * pw * 4), "store": DeviceBuffer(S * keys * 4),
           "monitor": DeviceBuffer(pw * 4), "mon_off": DeviceBuffer(S * (keys + 1) * 4), "err": DeviceBuffer(S * 4)}
    for b in out.values():
        b.fill_bytes(fill)
    inb = _lib.KvBatch(order.ptr, nexec.ptr, key.ptr, key_mask, ops.ptr, S, steps, keys, omax)
    outb = _lib.KvOut(out["result"].ptr, out["store"].ptr, out["monitor"].ptr, out["mon_off"].ptr, out["err"].ptr)
    if before_launch is not None:
        before_launch(None)
    check(lib.fx_kv_execute(ctypes.byref(inb), ctypes.byref(outb), None), "fx_kv_execute")
    check(lib.fx_dev_synchronize(None), "sync")
    return kv.KvResult(S, steps, keys, omax, out["result"].download(np.uint32, omax * pw),
                       out["store"].download(np.uint32, S * keys), out["monitor"].download(np.uint32, pw),
                       out["mon_off"].download(np.uint32, S * (keys + 1)), out["err"].download(np.uint32, S), 0,
                       out if keep_device else None)


def compare_monitors(a, rifl_a, b, rifl_b, pairs, before_launch=None, diff_pad=0):
    """fx_kv_monitor_compare (check_monitors over pairs of streams): a, b
    KvResults (their device buffers are used when run_kv kept them), rifl_*
    the planes naming the commands by arrival row (host arrays or
    DeviceBuffers), pairs [(stream of a, stream of b)].  Returns [(key,
    position)] per pair, (FX_KV_AGREE, FX_KV_AGREE) where the two agree.
    before_launch(stream): called right before the launch (tests: register
    poisoning).  diff_pad: `diff` is allocated that many words longer and
    starts as 0xA5 bytes; the call then returns (answers, the extra words as
    they are after the call)."""
    lib = _lib.load()
    keep = []
    pairs = np.ascontiguousarray(np.asarray(pairs, np.uint32).reshape(-1, 2))
    sides = []
    for r, rifl in ((a, rifl_a), (b, rifl_b)):
        mon, off = (r.dev["monitor"], r.dev["mon_off"]) if r.dev else (_dev(r.monitor, keep), _dev(r.mon_off, keep))
        sides.append(_lib.KvMonitor(mon.ptr, off.ptr, _dev(rifl, keep).ptr, r.S, r.steps, r.keys))
    diff = DeviceBuffer(pairs.nbytes + 4 * int(diff_pad))
    if diff_pad:
        diff.fill_bytes(0xA5)
    pairs_dev = _dev(pairs, keep)
    if before_launch is not None:
        before_launch(None)
    check(lib.fx_kv_monitor_compare(ctypes.byref(sides[0]), ctypes.byref(sides[1]), pairs_dev.ptr, len(pairs),
                                    diff.ptr, None), "fx_kv_monitor_compare")
    words = diff.download(np.uint32, pairs.size + int(diff_pad))
    answers = [(int(k), int(p)) for k, p in words[:pairs.size].reshape(-1, 2)]
    return (answers, words[pairs.size:]) if diff_pad else answers


def synth_kv_ops(seed, S, steps, read_pct=0, delete_pct=0, lengths=None, stream_base=0, before_launch=None):
    """fx_kv_synth_ops: one op plane generated on the device (lengths: None,
    a host array or a DeviceBuffer).  Returns the DeviceBuffer."""
    keep = []
    ops = DeviceBuffer(_lib.plane_words(S, steps) * 4)
    lengths = None if lengths is None else _dev(lengths, keep)
    if before_launch is not None:
        before_launch(None)
    check(_lib.load().fx_kv_synth_ops(seed, stream_base, read_pct, delete_pct, lengths.ptr if lengths else None, S,
                                      steps, ops.ptr, None), "fx_kv_synth_ops")
    check(_lib.load().fx_dev_synchronize(None), "sync")
    return ops


def run_pending(order, nexec, rifl, count, S, steps, count_mask=0xFFFFFFFF, process=0, fill=0, before_launch=None,
                tier=None, keep_device=False, stream_map=None):
    """AggregatePending over a batch: fx_pending_run (tier None: ONCHIP, then
    HBM for the streams that ran out of builders) or one fx_pending_aggregate
    at `tier` (FX_PENDING_TIER_*; stream_map: the streams of the launch, None =
    all).  order / nexec / rifl / count: host arrays or DeviceBuffers (the
    outputs of run_table(keep_device=True) and the planes of a DeviceTable are
    used where they are).  Every output, and the HBM tier's state, starts
    filled with the byte `fill`.  before_launch(stream): called right before
    the first launch (tests: register poisoning).  Returns a
    fantoch_amd.pending.PendingResult; a refused call raises, a stream's
    status lands in err."""
    from . import pending
    lib = _lib.load()
    keep = []
    order, nexec, rifl, count = (_dev(x, keep) for x in (order, nexec, rifl, count))
    pw = _lib.plane_words(S, steps)
    out = {name: DeviceBuffer(n * 4) for name, n in
           zip(pending.NAMES, (pending.MAX_PARTS * pw, pw, pw, pw, S, S, S))}
    for b in out.values():
        b.fill_bytes(fill)
    inb = _lib.PendingBatch(order.ptr, nexec.ptr, rifl.ptr, count.ptr, count_mask, process, S, steps)
    outb = _lib.PendingOut(*[out[name].ptr for name in pending.NAMES])
    reruns = ctypes.c_uint32()
    status = 0
    if tier is not None:
        lanes, dmap, state = S, None, None
        if stream_map is not None:
            lanes, dmap = len(stream_map), _dev(stream_map, keep)
        if tier == _lib.FX_PENDING_TIER_HBM:
            state = DeviceBuffer(lib.fx_pending_state_bytes(steps, lanes))
            state.fill_bytes(fill)
        if before_launch is not None:
            before_launch(None)
        check(lib.fx_pending_aggregate(ctypes.byref(inb), ctypes.byref(outb), dmap.ptr if dmap else None, lanes, tier,
                                       state.ptr if state else None, None), "fx_pending_aggregate")
        check(lib.fx_dev_synchronize(None), "sync")
    else:
        if before_launch is not None:
            before_launch(None)
        check(lib.fx_pending_run(ctypes.byref(inb), ctypes.byref(outb), None, ctypes.byref(reruns)), "fx_pending_run")
    res = pending.PendingResult(S, steps, *[out[name].download(np.uint32, out[name].nbytes // 4)
                                            for name in pending.NAMES], status, int(reruns.value),
                                out if keep_device else None)
    # what command_results needs beside the outputs: the rifl and the count of a head row
    res.rifl, res.count = rifl.download(np.uint32, pw), count.download(np.uint32, pw)
    res.count_mask, res.process = count_mask, process
    return res


class TableGroupResult:
    """Host copies of the outputs of fx_table_run_groups: the planes order,
    release, stable_sent, handled_src and handled_dot (steps_out rows), nexec,
    err and handled_len per stream, stable_clock [S, keys], rounds per group."""

    def __init__(self, S, steps_out, **arrays):
        self.S, self.steps_out = S, steps_out
        self.__dict__.update(arrays)

    def rows(self, name, s, count):
        """Rows 0..count-1 of stream s of the plane `name`."""
        return getattr(self, name)[_lib.index(np.arange(int(count)), s, self.steps_out)]


def _run_group_buffers(ins, S, steps, steps_out, n, keys, vmax, shards, targets_words, stability_threshold,
                       execute_at_commit, fill, max_rounds=None):
    """fx_table_run_groups (max_rounds: _capped) over inputs in device memory.
    ins: the DeviceBuffers hdr, dot, clock, votes, nkeys, route, targets and
    lengths; `state` and every output start filled with the byte `fill`.
    Returns the TableGroupResult."""
    lib = _lib.load()
    ow = _lib.plane_words(S, steps_out)
    outs = {name: DeviceBuffer(ow * 4) for name in ("order", "release", "stable_sent", "handled_src", "handled_dot")}
    outs.update({name: DeviceBuffer(S * 4) for name in ("nexec", "err", "handled_len")})
    outs["stable_clock"] = DeviceBuffer(S * keys * 4)
    outs["rounds"] = DeviceBuffer((S // shards if shards else 0) * 4)
    state = DeviceBuffer(lib.fx_table_groups_state_bytes(n, keys, S))
    for b in list(outs.values()) + [state]:
        b.fill_bytes(fill)
    inb = _lib.TableGroupBatch(
        _lib.TableBatchMk(_lib.TableBatch(ins["hdr"].ptr, ins["dot"].ptr, ins["clock"].ptr, ins["votes"].ptr,
                                          ins["lengths"].ptr, S, steps, n, keys, vmax, int(stability_threshold)),
                          ins["nkeys"].ptr),
        ins["route"].ptr, ins["targets"].ptr, targets_words, shards, steps_out)
    outb = _lib.TableGroupOut(_lib.OrderBatch(outs["order"].ptr, outs["release"].ptr, outs["nexec"].ptr,
                                              outs["err"].ptr), outs["stable_clock"].ptr, outs["stable_sent"].ptr,
                              outs["handled_src"].ptr, outs["handled_dot"].ptr, outs["handled_len"].ptr,
                              outs["rounds"].ptr)
    flags = _lib.FX_FLAG_EXECUTE_AT_COMMIT if execute_at_commit else 0
    if max_rounds is None:
        check(lib.fx_table_run_groups(ctypes.byref(inb), ctypes.byref(outb), state.ptr, flags, None),
              "fx_table_run_groups")
    else:
        check(lib.fx_table_run_groups_capped(ctypes.byref(inb), ctypes.byref(outb), state.ptr, flags, None,
                                             int(max_rounds)), "fx_table_run_groups_capped")
    check(lib.fx_dev_synchronize(None), "sync")
    got = {name: b.download(np.uint32, b.nbytes // 4) for name, b in outs.items()}
    got["stable_clock"] = got["stable_clock"].reshape(S, keys)
    return TableGroupResult(S, steps_out, **got)


def run_table_groups_packed(planes, route, targets, steps_out, shards, stability_threshold, execute_at_commit=False,
                            targets_words=None, fill=0xAB, max_rounds=None):
    """One fx_table_run_groups over what fantoch_amd.table.pack_table_groups
    returns.  targets_words: the value passed to the library (default: all of
    `targets`); fill: the byte that `state` and every output start filled
    with; max_rounds: a cap on the rounds instead of the library's own
    (fx_table_run_groups_capped, the library's hook for the tests of the cap).  Returns a TableGroupResult."""
    S = planes.S
    ins = {}
    for name, arr in (("hdr", planes.hdr), ("dot", planes.dot), ("clock", planes.clock), ("votes", planes.votes),
                      ("nkeys", planes.nkeys), ("route", route), ("targets", targets),
                      ("lengths", planes.lengths if planes.lengths is not None else np.full(S, planes.steps))):
        arr = np.ascontiguousarray(arr, np.uint32)
        ins[name] = DeviceBuffer(arr.nbytes)
        if arr.nbytes:
            ins[name].upload(arr)
    return _run_group_buffers(ins, S, planes.steps, int(steps_out), planes.n, planes.keys, planes.vmax, int(shards),
                              len(targets) if targets_words is None else int(targets_words), stability_threshold,
                              execute_at_commit, fill, max_rounds)


class DeviceTableGroups:
    """The input of fx_table_run_groups in device memory, filled by
    fx_table_group_synth_generate: S = groups * shards streams of up to `steps`
    rows (None: the longest stream, at least 1), vmax = fast_quorum vote slots,
    the nkeys and route planes, `targets_words` words of targets (None: what
    the lists take) and the lengths.  The constructor runs the counting pass
    (longest, steps_out, list_words); generate() fills the buffers; run() hands
    them to fx_table_run_groups with no host copy; download() gives what
    fantoch_amd.table.pack_table_groups returns."""
    ps = True

    def __init__(self, params, steps=None, targets_words=None):
        lib = _lib.load()
        self.params = params
        self.groups, self.shards = int(params.groups), int(params.shards)
        self.S, self.n, self.keys, self.vmax = self.groups * self.shards, int(params.n), int(params.keys), \
            int(params.fast_quorum)
        nbytes = lib.fx_table_group_synth_scratch_bytes(ctypes.byref(params))
        if nbytes == 0:
            raise _lib.FxError(_lib.FX_ERR_INVALID_ARG, "fx_table_group_synth_scratch_bytes")
        self.scratch = DeviceBuffer(nbytes)
        self.lengths = DeviceBuffer(self.S * 4)
        self.count()
        self.steps = max(self.longest, 1) if steps is None else int(steps)
        self.targets_words = self.list_words if targets_words is None else int(targets_words)
        self.plane = pw = _lib.plane_words(self.S, self.steps)
        self.bufs = {name: DeviceBuffer(pw * 4) for name in ("hdr", "dot", "clock", "nkeys", "route")}
        self.bufs["votes"] = DeviceBuffer(3 * self.vmax * pw * 4)
        self.bufs["targets"] = DeviceBuffer(self.targets_words * 4)

    def count(self):
        """fx_table_group_synth_count: sets longest, steps_out and list_words
        (the lengths stay on the device); returns the longest stream."""
        longest, steps_out, words = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
        check(_lib.load().fx_table_group_synth_count(ctypes.byref(self.params), self.lengths.ptr, self.scratch.ptr,
                                                     None, ctypes.byref(longest), ctypes.byref(steps_out),
                                                     ctypes.byref(words)), "fx_table_group_synth_count")
        self.longest, self.steps_out, self.list_words = longest.value, steps_out.value, words.value
        return self.longest

    def fill_bytes(self, value):
        """Every plane, targets and the lengths filled with one byte (tests: what a call leaves untouched)."""
        for b in list(self.bufs.values()) + [self.lengths]:
            b.fill_bytes(value)

    def generate(self):
        """fx_table_group_synth_generate into the buffers; returns the status."""
        b = self.bufs
        planes = _lib.TableGroupSynthPlanes(b["hdr"].ptr, b["dot"].ptr, b["clock"].ptr, b["votes"].ptr, b["nkeys"].ptr,
                                            b["route"].ptr, b["targets"].ptr, self.lengths.ptr)
        return _lib.load().fx_table_group_synth_generate(ctypes.byref(self.params), ctypes.byref(planes), self.steps,
                                                         self.targets_words, self.scratch.ptr, None)

    def _planes(self, S, lengths, get):
        from . import table
        p = table.TablePlanes(S, self.steps, self.n, self.keys, self.vmax, lengths=lengths)
        p.hdr, p.dot, p.clock, p.nkeys, route = (get(self.bufs[name], 1) for name in
                                                 ("hdr", "dot", "clock", "nkeys", "route"))
        p.votes = get(self.bufs["votes"], 3 * self.vmax)
        p.ps = True
        return p, route

    def download(self):
        """(planes, route, targets, steps_out), as fantoch_amd.table.pack_table_groups."""
        p, route = self._planes(self.S, self.lengths.download(np.uint32, self.S),
                                lambda buf, k: buf.download(np.uint32, k * self.plane))
        return p, route, self.bufs["targets"].download(np.uint32, self.targets_words), self.steps_out

    def download_tile(self, tile):
        """The 64 streams of plane tile `tile` as (planes, route): stream s of
        the launch is stream s % 64 of tile s // 64; the route rows index the
        whole targets array."""
        S, lengths, part = _tile_download(self.lengths, self.S, self.plane, self.steps, tile)
        got = self._planes(S, lengths, part)
        check(_lib.load().fx_dev_synchronize(None), "fx_dev_synchronize")
        return got

    def run(self, stability_threshold, execute_at_commit=False, fill=0xAB):
        """fx_table_run_groups over the generated buffers, as
        run_table_groups_packed over a host copy of them (`state` and every
        output start filled with the byte `fill`).  Returns a TableGroupResult."""
        return _run_group_buffers(dict(self.bufs, lengths=self.lengths), self.S, self.steps, self.steps_out, self.n,
                                  self.keys, self.vmax, self.shards, self.targets_words, stability_threshold,
                                  execute_at_commit, fill)


def synth_table_groups(params, steps=None, targets_words=None, before_launch=None):
    """Closed-loop shard groups generated on the device
    (fx_table_group_synth_generate; fantoch_amd.table.table_group_synth_params):
    returns the DeviceTableGroups holding them.  before_launch(stream): called
    right before the generator's launches (tests: register poisoning)."""
    t = DeviceTableGroups(params, steps, targets_words)
    if before_launch is not None:
        before_launch(None)
    check(t.generate(), "fx_table_group_synth_generate")
    return t


def run_table_groups(groups, n, keys, stability_threshold, delay=None, execute_at_commit=False):
    """fantoch_amd.table.run_table_groups with the closed loop inside one
    kernel launch (fx_table_run_groups): the same arguments, the same
    delivery rule and exactly the same return value -- per
    group `streams` (the events as handled, rebuilt from the handled_src and
    handled_dot planes and the own events), `results` (order, release, sent,
    nexec, err, stable per shard) and `rounds`."""
    from . import table
    planes, route, targets, steps_out = table.pack_table_groups(groups, n, keys, delay)
    if planes.S == 0:
        return []
    P = len(groups[0][0])
    res = run_table_groups_packed(planes, route, targets, steps_out, P, stability_threshold, execute_at_commit)
    return table_group_dicts(groups, res)


def table_group_dicts(groups, res):
    """A TableGroupResult as fantoch_amd.table.run_table_groups returns the
    closed loop of `groups`: one dict (streams, results, rounds) per group."""
    from . import table
    P = len(groups[0][0])
    out = []
    for i, (own, _) in enumerate(groups):
        streams, results = [], []
        for h in range(P):
            s = i * P + h
            L, nexec = int(res.handled_len[s]), int(res.nexec[s])
            streams.append(table.handled_stream(own[h], res.rows("handled_src", s, L), res.rows("handled_dot", s, L)))
            planes_ = {name: {a: int(v) for a, v in enumerate(res.rows(name, s, L)) if v != _lib.FX_RELEASE_NONE}
                       for name in ("release", "stable_sent")}
            order = [int(x) & ~_lib.FX_ORDER_SCC_START for x in res.rows("order", s, nexec)]
            results.append(dict(order=order, release=planes_["release"], sent=planes_["stable_sent"], nexec=nexec,
                                err=int(res.err[s]), stable=[int(x) for x in res.stable_clock[s]]))
        out.append(dict(streams=streams, results=results, rounds=int(res.rounds[i])))
    return out


class TableSession:
    """Tempo's TableExecutor fed in pieces (fx_table_advance, HBM-tier tables):
    owns the device planes, the outputs and the state of S streams of up to
    `steps` rows for its lifetime.  kind: FX_TABLE_KIND_* (the semantics of
    fx_table_execute, _mk or _ps).  The order plane starts filled with the byte
    order_fill, the release and stable_sent planes with FX_RELEASE_NONE."""

    def __init__(self, S, steps, n, keys, vmax, stability_threshold, kind, execute_at_commit=False, order_fill=0):
        lib = _lib.load()
        self.S, self.steps, self.n, self.keys, self.vmax = int(S), int(steps), int(n), int(keys), int(vmax)
        self.thr, self.kind, self.at_commit = int(stability_threshold), int(kind), bool(execute_at_commit)
        self.plane = pw = _lib.plane_words(self.S, self.steps)
        self.bufs = {name: DeviceBuffer(pw * 4) for name in ("hdr", "dot", "clock")}
        self.bufs["votes"] = DeviceBuffer(3 * self.vmax * pw * 4)
        self.nkeys = None
        if kind != _lib.FX_TABLE_KIND_SINGLE:  # until the planes bring their own: one key (and one shard) each
            self.nkeys = DeviceBuffer(pw * 4)
            self.nkeys.upload(np.full(pw, 0x101 if kind == _lib.FX_TABLE_KIND_PS else 1, np.uint32))
        self.lengths = DeviceBuffer(self.S * 4)
        self.order, self.release = DeviceBuffer(pw * 4), DeviceBuffer(pw * 4)
        self.order_fill = order_fill
        self.order.fill_bytes(order_fill)
        self.release.fill_bytes(0xFF)
        self.sent = None
        if kind == _lib.FX_TABLE_KIND_PS:
            self.sent = DeviceBuffer(pw * 4)
            self.sent.fill_bytes(0xFF)
        self.nexec, self.err = DeviceBuffer(self.S * 4), DeviceBuffer(self.S * 4)
        self.nexec.fill_bytes(0xAB)
        self.err.fill_bytes(0xAB)
        self.stable = DeviceBuffer(self.S * self.keys * 4)
        self.stable.fill_bytes(0xAB)
        self.state_bytes = lib.fx_table_session_bytes(self.kind, self.n, self.keys, self.S)
        self.state = DeviceBuffer(self.state_bytes)
        self.done = np.zeros(self.S, np.uint32)  # rows on the device and handed to the executor
        self.started = False

    def reset(self):
        """The next advance starts every stream again from an empty executor
        at row 0 (FX_FLAG_INIT); the outputs are filled as at the start."""
        self.done[:] = 0
        self.started = False
        self.order.fill_bytes(self.order_fill)
        self.release.fill_bytes(0xFF)
        if self.sent is not None:
            self.sent.fill_bytes(0xFF)

    def upload(self, planes, lengths):
        """Copies the 4-step tile rows that hold rows [done, lengths) of each
        stream: per 64-stream tile, every run of adjacent such tile rows is
        one copy per plane."""
        pw, steps4 = self.plane, (self.steps + 3) // 4
        arrays = [(self.bufs["hdr"], planes.hdr, 0), (self.bufs["dot"], planes.dot, 0),
                  (self.bufs["clock"], planes.clock, 0)]
        arrays += [(self.bufs["votes"], planes.votes, p * pw) for p in range(3 * self.vmax)]
        if self.nkeys is not None and planes.nkeys is not None:
            arrays.append((self.nkeys, planes.nkeys, 0))
        for tile in range((self.S + 63) // 64):
            sl = slice(tile * 64, min(self.S, tile * 64 + 64))
            grow = lengths[sl] > self.done[sl]
            if not grow.any():
                continue
            new = np.zeros(steps4 + 2, bool)  # tile row t at [t + 1]
            for d, l in zip(self.done[sl][grow], lengths[sl][grow]):
                new[(int(d) >> 2) + 1:((int(l) - 1) >> 2) + 2] = True
            edges = np.flatnonzero(new[1:] != new[:-1])  # starts and ends of the runs, alternating
            for t0, t1 in zip(edges[0::2], edges[1::2]):
                lo, hi = (tile * steps4 + int(t0)) * 256, (tile * steps4 + int(t1)) * 256
                for buf, arr, base in arrays:
                    buf.upload_at((base + lo) * 4, np.asarray(arr[base + lo:base + hi], np.uint32))
        self.lengths.upload(lengths)

    def launch(self, init=False, steps=None, stability_threshold=None):
        """One fx_table_advance over what is on the device.  steps,
        stability_threshold: values other than the session's (a call that
        breaks the session contract)."""
        inb = _lib.TableBatchMk(
            _lib.TableBatch(self.bufs["hdr"].ptr, self.bufs["dot"].ptr, self.bufs["clock"].ptr,
                            self.bufs["votes"].ptr, self.lengths.ptr, self.S,
                            self.steps if steps is None else int(steps), self.n, self.keys, self.vmax,
                            self.thr if stability_threshold is None else int(stability_threshold)),
            self.nkeys.ptr if self.nkeys else None)
        outb = _lib.OrderBatch(self.order.ptr, self.release.ptr, self.nexec.ptr, self.err.ptr)
        flags = (_lib.FX_FLAG_INIT if init else 0) | (_lib.FX_FLAG_EXECUTE_AT_COMMIT if self.at_commit else 0)
        check(_lib.load().fx_table_advance(ctypes.byref(inb), self.kind, ctypes.byref(outb), self.stable.ptr,
                                           self.sent.ptr if self.sent else None, self.state.ptr, flags, None),
              "fx_table_advance")

    def result(self):
        """Host copies of the outputs as they are now (a TableResult)."""
        pw, S = self.plane, self.S
        return TableResult(self.order.download(np.uint32, pw), self.release.download(np.uint32, pw),
                           self.nexec.download(np.uint32, S), self.err.download(np.uint32, S),
                           self.stable.download(np.uint32, S * self.keys).reshape(S, self.keys), 0, 0,
                           self.sent.download(np.uint32, pw) if self.sent is not None else None)

    def advance(self, planes, **contract):
        """Hands the executor rows [done, planes.lengths) of every stream of
        the host TablePlanes (lengths None = all `steps` rows; lengths do not
        decrease from call to call) and returns the outputs so far.  The first
        call starts the streams (FX_FLAG_INIT).  contract: see launch()."""
        if (planes.S, planes.steps, planes.n, planes.keys, planes.vmax) != \
                (self.S, self.steps, self.n, self.keys, self.vmax):
            raise ValueError("TableSession.advance: planes of another shape than the session's")
        lengths = np.full(self.S, self.steps, np.uint32) if planes.lengths is None \
            else np.ascontiguousarray(planes.lengths, np.uint32)
        self.upload(planes, lengths)
        self.launch(init=not self.started, **contract)
        self.started = True
        if not contract:
            self.done = np.maximum(self.done, lengths)
        return self.result()
