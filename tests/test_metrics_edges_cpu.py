"""The metrics pass without a GPU: the host twin (fx_batch_metrics_host) against the restatement on every
edge case of metrics_edges at every bin pair, whole buffers with the guard word behind each histogram; bins that
hold something before the call; every refusal of fx_batch_metrics and of the twin; and the stand-alone
sanitizer run of the twin.  CPU only."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import metrics_edges as E
from fantoch_amd import _lib
from fantoch_amd import metrics as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, IDS = E.params()


def same(got, want, what):
    """Whole buffers: the bins and the guard word behind them."""
    for name, g, w in zip(("ChainSize", "ExecutionDelay"), got, want):
        assert len(g) == len(w) + 1 and int(g[-1]) == fm.GUARD, "%s: %s guard word" % (what, name)
        assert np.array_equal(g[:-1], w), "%s: %s differs at bin %d" % (what, name, int(np.flatnonzero(g[:-1] != w)[0]))


def run_host(c, nbc, nbd, chain0=None, delay0=None):
    return fm.run_metrics_host(c.hdr, c.order, c.release, c.nexec, c.S, c.steps, nbc, nbd, chain0, delay0)


@pytest.mark.parametrize("name,nbc,nbd", ROWS, ids=IDS)
def test_host_twin_matches_the_restatement(name, nbc, nbd):
    c = E.case(name, nbc, nbd)
    same(run_host(c, nbc, nbd), c.expected(nbc, nbd), name)


@pytest.mark.parametrize("name", E.ACCUMULATE)
@pytest.mark.parametrize("nbc,nbd", E.PAIRS)
def test_host_twin_accumulates(name, nbc, nbd):
    """Bins that start at 1, 2^32 - 1 and 2^40; a second call over the result doubles the increments."""
    c = E.case(name, nbc, nbd)
    chain0, delay0 = E.start_bins(nbc), E.start_bins(nbd)
    once = run_host(c, nbc, nbd, chain0, delay0)
    same(once, c.expected(nbc, nbd, chain0, delay0), name)
    twice = run_host(c, nbc, nbd, once[0][:-1], once[1][:-1])
    same(twice, c.expected(nbc, nbd, chain0, delay0, calls=2), name)
    added = [int((b[:-1] - a).sum()) for a, b in zip((chain0, delay0), twice)]
    assert added == [2 * len(c.samples()[1]), 2 * len(c.samples()[0])] and added[1] > 0


def test_empty_batches_leave_the_histograms_alone():
    for name in ("empty 0x8", "empty 8x0"):
        c = E.case(name, 2, 2)
        start = E.start_bins(2)
        same(run_host(c, 2, 2, start, start), (start, start), name)


def test_symbols_are_bound(lib):
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for name in ("fx_batch_metrics", "fx_batch_metrics_host"):
        assert hasattr(lib, name) and name in bound


# ------------------------------------------------------------------ refusals
def call(lib, fn, bufs, null=None, **over):
    """One call over the buffers; null: the struct or plane passed as NULL; over: nbins_chain / nbins_delay."""
    p = {k: (None if k == null else v.ctypes.data) for k, v in bufs.items()}
    inb = _lib.StreamBatch(None, p["hdr"], None, None, 2, 8, 0, 0)
    outb = _lib.OrderBatch(p["order"], p["release"], p["nexec"], None)
    hb = _lib.HistBatch(p["chain"], over.get("nbins_chain", 4), p["delay"], over.get("nbins_delay", 4))
    args = [None if null == n else ctypes.byref(x) for n, x in (("in", inb), ("out", outb), ("hists", hb))]
    return getattr(lib, fn)(*args, *(() if fn.endswith("_host") else (None,)))


REFUSED = [dict(null=n) for n in ("in", "out", "hists", "hdr", "order", "release", "nexec", "chain", "delay")] + \
    [dict(nbins_chain=0), dict(nbins_chain=1), dict(nbins_delay=0), dict(nbins_delay=1)]


@pytest.mark.parametrize("fn", ["fx_batch_metrics_host", "fx_batch_metrics"])
def test_refused_calls_write_nothing(lib, fn):
    """Before the library looks for a device: FX_ERR_INVALID_ARG with or without a GPU, and nothing is launched
    (the pointers are host memory)."""
    c = E.case("narrow tails 5x7", 2, 2)
    bufs = dict(hdr=c.hdr, order=c.order, release=c.release, nexec=c.nexec[:2].copy(),
                chain=np.full(5, 7, np.uint64), delay=np.full(5, 7, np.uint64))
    for how in REFUSED:
        assert call(lib, fn, bufs, **how) == _lib.FX_ERR_INVALID_ARG, how
        assert np.all(bufs["chain"] == 7) and np.all(bufs["delay"] == 7), how
    assert getattr(lib, fn)(None, None, None, *(() if fn.endswith("_host") else (None,))) == _lib.FX_ERR_INVALID_ARG


def test_the_device_call_needs_a_device(lib):
    if lib.fx_device_count() > 0:
        pytest.skip("a GPU is visible")
    c = E.case("narrow tails 5x7", 2, 2)
    bufs = dict(hdr=c.hdr, order=c.order, release=c.release, nexec=c.nexec,
                chain=np.full(5, 7, np.uint64), delay=np.full(5, 7, np.uint64))
    assert call(lib, "fx_batch_metrics", bufs) == _lib.FX_ERR_NO_DEVICE
    assert np.all(bufs["chain"] == 7) and np.all(bufs["delay"] == 7)


def test_the_valid_host_call(lib):
    """The arguments the refusals start from are good: 2 streams of 8 rows over the planes of a 5 x 7 case."""
    c = E.case("narrow tails 5x7", 2, 2)
    bufs = dict(hdr=c.hdr, order=c.order, release=c.release, nexec=c.nexec[:2].copy(),
                chain=np.zeros(5, np.uint64), delay=np.zeros(5, np.uint64))
    assert call(lib, "fx_batch_metrics_host", bufs) == _lib.FX_OK
    assert bufs["delay"][:4].sum() == c.nexec[:2].sum() and bufs["delay"][4] == 0 and bufs["chain"][4] == 0


# ------------------------------------------------------------------ sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_twin_under_the_sanitizers():
    out = subprocess.run(["make", "-C", ROOT, "metrics-check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "metrics_host_check: ok" in out.stdout
