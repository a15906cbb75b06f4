"""fx_batch_metrics (k_metrics) on every edge case of metrics_edges at every bin pair: against the restatement
(metrics_ref), against the host twin, and the LDS path against the global-atomics path.  dot, deps and lengths
are null, the histograms have exactly nbins words and a guard word behind them.  Each case's planes go to the
device once.  GPU only."""
import functools

import numpy as np
import pytest

import metrics_edges as E
from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import metrics as fm

pytestmark = pytest.mark.gpu
ROWS, IDS = E.params()


@functools.lru_cache(maxsize=4)
def on_device(c):
    """The case's planes on the device (cases are kept by identity: metrics_edges builds each once)."""
    keep = []
    return tuple(fd._dev(x, keep) for x in (c.hdr, c.order, c.release, c.nexec))


def run(c, nbc, nbd, chain0=None, delay0=None):
    return fd.run_metrics(*on_device(c), c.S, c.steps, nbc, nbd, chain0, delay0)


def same(got, want, what):
    """Whole buffers: the bins and the guard word behind them."""
    for name, g, w in zip(("ChainSize", "ExecutionDelay"), got, want):
        assert len(g) == len(w) + 1 and int(g[-1]) == fm.GUARD, "%s: %s guard word" % (what, name)
        assert np.array_equal(g[:-1], w), "%s: %s differs at bin %d" % (what, name, int(np.flatnonzero(g[:-1] != w)[0]))


@pytest.mark.parametrize("name,nbc,nbd", ROWS, ids=IDS)
def test_device_matches_the_restatement_and_the_host_twin(gpu, name, nbc, nbd):
    c = E.case(name, nbc, nbd)
    got = run(c, nbc, nbd)
    same(got, c.expected(nbc, nbd), name)
    host = fm.run_metrics_host(c.hdr, c.order, c.release, c.nexec, c.S, c.steps, nbc, nbd)
    assert all(np.array_equal(g, h) for g, h in zip(got, host)), name


@pytest.mark.parametrize("name", E.NAMES)
def test_lds_and_global_atomics_agree(gpu, name):
    """The last pair that counts in LDS and the first that does not: the same bins, byte for byte, the one more
    bin of the second apart (the case's own planes where they depend on the pair: the same input to both)."""
    (nbc, nbd), (gbc, gbd) = E.PAIRS[2], E.PAIRS[3]
    assert E.uses_lds(nbc, nbd) and not E.uses_lds(gbc, gbd) and (gbc, gbd) == (nbc, nbd + 1)
    for pair in (E.PAIRS[2], E.PAIRS[3]):
        c = E.case(name, *pair)
        lds, glob = run(c, nbc, nbd), run(c, gbc, gbd)
        assert lds[0].tobytes() == glob[0].tobytes(), name
        # the last LDS bin holds what the two last global bins hold
        assert lds[1][:nbd - 1].tobytes() == glob[1][:nbd - 1].tobytes(), name
        assert int(lds[1][nbd - 1]) == int(glob[1][nbd - 1]) + int(glob[1][nbd]), name
        # and with equal bin counts on both paths: 63 chain bins take the LDS pair's size to the limit's other side
        same_bins = run(c, nbc + 1, nbd)
        assert not E.uses_lds(nbc + 1, nbd) and same_bins[1].tobytes() == lds[1].tobytes(), name


@pytest.mark.parametrize("name", E.ACCUMULATE)
@pytest.mark.parametrize("nbc,nbd", E.PAIRS)
def test_device_accumulates(gpu, name, nbc, nbd):
    """Bins that start at 1, 2^32 - 1 and 2^40; a second call over the result doubles the increments."""
    c = E.case(name, nbc, nbd)
    chain0, delay0 = E.start_bins(nbc), E.start_bins(nbd)
    once = run(c, nbc, nbd, chain0, delay0)
    same(once, c.expected(nbc, nbd, chain0, delay0), name)
    twice = run(c, nbc, nbd, once[0][:-1], once[1][:-1])
    same(twice, c.expected(nbc, nbd, chain0, delay0, calls=2), name)


def test_empty_batches_leave_the_histograms_alone(gpu):
    for name in ("empty 0x8", "empty 8x0"):
        c = E.case(name, 2, 2)
        start = E.start_bins(2)
        same(run(c, 2, 2, start, start), (start, start), name)


def test_run_batch_goes_through_run_metrics(gpu):
    """run_batch's histograms are run_metrics' over its own outputs."""
    from fantoch_amd import streams as fs
    planes = fs.synth_host(fs.synth_params(seed=3, instances=5, n=3, cmds=30, window=4, cycle_pct=30))
    res = fd.run_batch(planes, nbins_chain=8, nbins_delay=64)
    chain, delay = fd.run_metrics(planes.hdr, res.order, res.release, res.nexec, planes.S, planes.steps, 8, 64)
    assert np.array_equal(res.chain, chain[:-1]) and np.array_equal(res.delay, delay[:-1])
    assert int(delay[-1]) == fm.GUARD and res.delay.sum() == res.nexec.sum()
