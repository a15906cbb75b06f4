"""Statistics of the reduced dense histograms (Histogram, fantoch/src/metrics/histogram.rs).

The batched executor folds ChainSize / ExecutionDelay samples into dense bins
(k_metrics, all-reduced across ranks); this turns a dense count array into the
reference's `Histogram` statistics through the C-ABI: mean / stddev / cov / mdtm
(histogram.rs:61-110, 172-235, fx_hist_stats_compute) and percentiles
(histogram.rs:111-170, fx_hist_percentile).  The last bin holds every value
>= nbins - 1, so statistics are exact only when it is empty (`clamped` == 0).

run_metrics_host is the metrics pass itself over host memory
(fx_batch_metrics_host, the host twin of fx_batch_metrics; the device side:
fantoch_amd.device.run_metrics).  Both runners hand the library histograms of
exactly nbins words with one guard word behind each and return the two buffers
whole, guard included.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check


def dense_stats(counts, percentiles=(0.5, 0.95, 0.99)):
    counts = np.ascontiguousarray(np.asarray(counts, dtype=np.uint64))
    nz = np.flatnonzero(counts)
    values = np.ascontiguousarray(nz.astype(np.uint64))
    cnts = np.ascontiguousarray(counts[nz])
    out = {"count": int(cnts.sum()), "clamped": int(counts[-1]) if len(counts) else 0}
    if not len(nz):
        return out
    u64p = ctypes.POINTER(ctypes.c_uint64)
    vp, cp = values.ctypes.data_as(u64p), cnts.ctypes.data_as(u64p)
    lib = _lib.load()
    st = _lib.HistStats()
    check(lib.fx_hist_stats_compute(vp, cp, len(nz), ctypes.byref(st)), "fx_hist_stats_compute")
    out.update(mean=st.mean, stddev=st.stddev, cov=st.cov, mdtm=st.mdtm, min=st.min, max=st.max)
    for p in percentiles:
        r = ctypes.c_double()
        check(lib.fx_hist_percentile(vp, cp, len(nz), p, ctypes.byref(r)), "fx_hist_percentile")
        out["p%g" % (p * 100)] = r.value
    return out


GUARD = 0xA5A5A5A5A5A5A5A5  # the word behind each histogram: a call must leave it alone


def guarded(nbins, start=None):
    """A histogram buffer of nbins words (start: their values, None = zeros) and the guard word."""
    buf = np.zeros(int(nbins) + 1, np.uint64)
    if start is not None:
        buf[:-1] = np.asarray(start, np.uint64)
    buf[-1] = GUARD
    return buf


def run_metrics_host(hdr, order, release, nexec, S, steps, nbins_chain, nbins_delay, chain0=None, delay0=None):
    """fx_batch_metrics_host over host arrays; dot, deps and lengths are null.
    The bins start at chain0 / delay0 (None: zero).  Returns (chain, delay),
    each with its guard word as the last element; a refused call raises."""
    hdr, order, release, nexec = (np.ascontiguousarray(x, np.uint32) for x in (hdr, order, release, nexec))
    chain, delay = guarded(nbins_chain, chain0), guarded(nbins_delay, delay0)
    inb = _lib.StreamBatch(None, hdr.ctypes.data, None, None, S, steps, 0, 0)
    outb = _lib.OrderBatch(order.ctypes.data, release.ctypes.data, nexec.ctypes.data, None)
    hb = _lib.HistBatch(chain.ctypes.data, nbins_chain, delay.ctypes.data, nbins_delay)
    check(_lib.load().fx_batch_metrics_host(ctypes.byref(inb), ctypes.byref(outb), ctypes.byref(hb)),
          "fx_batch_metrics_host")
    return chain, delay
