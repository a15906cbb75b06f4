"""A plain restatement of the metrics pass (fx_batch_metrics, include/fantoch_amd.h) over host planes.

For stream s, ne = nexec[s]; a stream with ne > steps gives nothing.  For each order row k < ne, with
rec = order[k] & 0x7FFFFFFF and rs = release[rec] (looked up only if rec < steps):
  - the row gives a delay sample iff rec < steps and rs < steps: (t(hdr[rs]) - t(hdr[rec])) mod 2^32 with
    t = the low 24 bits of a header, so a release before the arrival wraps to a value near 2^32;
  - a row that gives a delay sample and carries bit 31 also gives one chain sample: 1 + the rows without
    bit 31 that follow it below ne.
A sample v lands in bin min(v, nbins - 1).  Everything is int64; the wrap is the one `& U32` below."""
import numpy as np

from fantoch_amd import _lib

U32 = 0xFFFFFFFF
REC_MASK = 0x7FFFFFFF
T_MASK = 0x00FFFFFF


def stream_samples(hdr, order, release, ne, s, steps):
    """(delays, sizes) of one stream that executed ne rows: int64 arrays of the unclamped samples."""
    none = np.zeros(0, np.int64)
    if ne > steps or ne == 0:
        return none, none
    o = order[_lib.index(np.arange(ne), s, steps)].astype(np.int64)
    rec = o & REC_MASK
    flagged = (o >> 31) & 1 == 1
    counts = rec < steps
    rs = np.full(ne, _lib.FX_RELEASE_NONE, np.int64)
    rs[counts] = release[_lib.index(rec[counts], s, steps)]
    counts &= rs < steps
    t = lambda rows: hdr[_lib.index(rows, s, steps)].astype(np.int64) & T_MASK
    delays = (t(rs[counts]) - t(rec[counts])) & U32  # the u32 wrap
    sizes = []
    for k in np.flatnonzero(flagged & counts):
        size = 1
        while k + size < ne and not flagged[k + size]:
            size += 1
        sizes.append(size)
    return delays, np.asarray(sizes, np.int64)


def samples(hdr, order, release, nexec, S, steps, streams=None):
    """(delays, sizes) of the streams (None: all S)."""
    parts = [stream_samples(hdr, order, release, int(nexec[s]), s, steps)
             for s in (range(S) if streams is None else streams)]
    parts.append((np.zeros(0, np.int64),) * 2)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def bins(values, nbins, start=None):
    """The histogram of nbins words (uint64) after the samples are added to `start` (None: zeros)."""
    hist = np.zeros(nbins, np.uint64) if start is None else np.array(start, np.uint64)
    assert len(hist) == nbins
    hist += np.bincount(np.minimum(values, nbins - 1), minlength=nbins).astype(np.uint64)  # wraps like a uint64_t
    return hist


def hists(hdr, order, release, nexec, S, steps, nbc, nbd, streams=None):
    """(chain, delay): what fx_batch_metrics adds to zeroed histograms of nbc and nbd bins."""
    delays, sizes = samples(hdr, order, release, nexec, S, steps, streams)
    return bins(sizes, nbc), bins(delays, nbd)
