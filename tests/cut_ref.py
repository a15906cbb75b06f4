"""The quiescent-cut analysis of fantoch_amd/csrc/graph_cut.hip restated (test
infrastructure): numpy over a host `Planes`, no call into the library.

What fx_batch_run_cut decides before and around the batched executor is
restated here as plainly as it can be said -- one sort for the position table,
one prefix maximum, one pass over the cuts -- so that the driver's twenty
kernels, three round trips and two-level scans can be held against it:

  per stream   reach, the cut flags, the segments (a, b), each segment's
               length class, and why a stream is not cut (REASONS);
  per batch    what fx_cut_stats must report (segments, single_segments,
               max_segment, whole_streams), the batch slots the segment batch
               has (h_nbatch), nch, which chunk-scan kernel and which rank
               kernel run, and whether the sparse-seq fallback is taken;
  per segment  the renumbered stream k_build hands the batched executor
               (renumber), and its outputs mapped back (tests only).

The constants are read from the text of graph_cut.hip (constant()), so a
changed limit moves the cases of cut_edges with it or fails their checks:
  INF, MAX_SEG, CHUNK, BT    the head of namespace fx::cut
  SMALL_S                    above k_part_max (part + k_part_max against flush_block)
  NCLS                       above seg_class
  RANK_INLINE, RANK_CLASS_MIN  above k_rank_slots
  the 64 of `nch > 64`       chunk_excl() (BLK_ABOVE)
  FX_TILE_STREAMS            include/fantoch_amd.h (item(): plane order up to one tile column)
  the 2^32 of `ptotal > (1ull << 32)` and the 8 of `nl_adds * 8 < work`:
                             fx_batch_run_cut (SPARSE_ABOVE, RANK_SLOTS_FACTOR)

Deliberately wrong variants (test_cut_edges_ref.py shows that each case of
cut_edges tells them from the right one): analyse(no_carry=CHUNK) forgets the
block-exclusive carry (cmax_excl), no_carry=CHUNK * CHUNK the carry between
the rounds of k_chunk_excl_blk, max_seg moves MAX_SEG, singles="all" counts
the one-Add segments of every stream (what the driver did before), and
renumber(by_source=False) ranks a dot among all the segment's dots.
"""
import os
import re

import numpy as np

from fantoch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TEXT = {}


def constant(name, path="fantoch_amd/csrc/graph_cut.hip", pattern=None):
    """The value of `constexpr uint32_t name = value;` (or of `pattern`'s group) in the source's text."""
    if path not in _TEXT:
        with open(os.path.join(ROOT, path)) as f:
            _TEXT[path] = f.read()
    m = re.search(pattern or r"constexpr uint32_t %s = (\w+);" % name, _TEXT[path])
    assert m, "%s not found in %s" % (name, path)
    return int(m.group(1).rstrip("u"), 0)


INF = constant("INF")
MAX_SEG = constant("MAX_SEG")
CHUNK = constant("CHUNK")
BT = constant("BT")
SMALL_S = constant("SMALL_S")
NCLS = constant("NCLS")
RANK_INLINE = constant("RANK_INLINE")
RANK_CLASS_MIN = constant("RANK_CLASS_MIN")
BLK_ABOVE = constant("nch > N", pattern=r"if \(nch > (\d+)\) hipLaunchKernelGGL\(k_chunk_excl_blk")
SPARSE_ABOVE = 1 << constant("ptotal", pattern=r"if \(ptotal > \(1ull << (\d+)\)\) return run_tiered")
RANK_SLOTS_FACTOR = constant("nl_adds", pattern=r"if \(nl_adds \* (\d+) < work\)")
TILE_STREAMS = constant("FX_TILE_STREAMS", "include/fantoch_amd.h", r"#define FX_TILE_STREAMS (\d+)u")
OVER = 13  # seg_class: the class of a segment over MAX_SEG
assert CHUNK == 4 * BT and MAX_SEG == 1 << 12 and SMALL_S == TILE_STREAMS

# why a stream runs whole, in the order the driver meets them
BAD_SOURCE, DOUBLE_DOT, NOT_AN_ADD, NO_FINAL_CUT, OVER_MAX_SEG = \
    "dot source outside 1..n", "double dot", "record that is not an Add", "no cut at the last step", \
    "segment over MAX_SEG"
BAD = (BAD_SOURCE, DOUBLE_DOT, NOT_AN_ADD)  # the stream's `bad` word (k_maxseq, k_pos, k_reach)


def seg_class(length, max_seg=MAX_SEG):
    """seg_class(): 0 for a single, ceil(log2 length) up to MAX_SEG, 13 beyond."""
    if length < 2:
        return 0
    return OVER if length > max_seg else int(length - 1).bit_length()


def prefix_max(v, no_carry=None):
    if not no_carry:
        return np.maximum.accumulate(v)
    out = np.empty_like(v)
    for b in range(0, len(v), no_carry):
        out[b:b + no_carry] = np.maximum.accumulate(v[b:b + no_carry])
    return out


class StreamCut:
    """One stream's analysis: L, dot, nd, deps [dmax, L], reach, flags, the segments (start, end, length, cls
    arrays, in order) and reasons (empty: the stream is cut)."""

    def __init__(self, planes, s, no_carry=None, max_seg=MAX_SEG):
        steps, n, dmax = planes.steps, planes.n, planes.dmax
        self.s, self.n = s, n
        self.L = L = steps if planes.lengths is None else min(int(planes.lengths[s]), steps)
        at = _lib.index(np.arange(L), s, steps)
        self.dot, hdr = planes.dot[at], planes.hdr[at]
        self.nd = np.minimum((hdr >> 24) & 31, dmax).astype(np.int64)
        self.deps = planes.deps.reshape(max(dmax, 1), planes.plane)[:dmax][:, at] if L else np.zeros((dmax, 0), np.uint32)
        src = self.dot >> _lib.FX_SEQ_BITS
        ok = (src >= 1) & (src <= n)
        # the position table (k_pos): the stream's dots of a source in 1..n, by dot
        by_dot = np.argsort(self.dot[ok], kind="stable")
        self.table, self.table_pos = self.dot[ok][by_dot], np.flatnonzero(ok)[by_dot]
        self.reasons = []
        if not ok.all():
            self.reasons.append(BAD_SOURCE)
        if np.any(self.table[1:] == self.table[:-1]):
            self.reasons.append(DOUBLE_DOT)
        if np.any((hdr >> 29) != _lib.FX_KIND_ADD):
            self.reasons.append(NOT_AN_ADD)
        # reach (k_reach): max(i, the position of each of the first min(nd, dmax) deps), INF for one never added
        self.reach = np.arange(L, dtype=np.int64)
        for j in range(dmax):
            rows = np.flatnonzero(self.nd > j)
            if len(rows):
                self.reach[rows] = np.maximum(self.reach[rows], self.position(self.deps[j][rows]))
        # cut flags (k_chunk_max, k_chunk_excl*, k_flags): prefix max of reach <= i
        self.flags = prefix_max(self.reach, no_carry) <= np.arange(L)
        self.end = np.flatnonzero(self.flags)
        self.start = np.concatenate(([0], self.end[:-1] + 1)) if len(self.end) else self.end
        self.length = self.end - self.start + 1
        self.cls = np.array([seg_class(int(x), max_seg) for x in self.length], np.int64)
        if L and not self.flags[-1]:
            self.reasons.append(NO_FINAL_CUT)
        if len(self.length) and self.length.max() > max_seg:
            self.reasons.append(OVER_MAX_SEG)
        self.whole = bool(self.reasons)
        self.bad = any(r in BAD for r in self.reasons)
        self.max_seq = int((self.dot & _lib.FX_SEQ_MASK).max()) if L else 0  # k_maxseq: every dot, whatever its source

    def position(self, dots):
        """The step of each dot (INF: not among the stream's dots below its length)."""
        if not len(self.table):
            return np.full(len(dots), INF, np.int64)
        k = np.minimum(np.searchsorted(self.table, dots), len(self.table) - 1)
        return np.where(self.table[k] == dots, self.table_pos[k], INF).astype(np.int64)

    @property
    def segments(self):
        return list(zip(self.start.tolist(), self.end.tolist()))

    def singles(self):
        return int((self.length == 1).sum())

    def renumber(self, k, by_source=True):
        """Segment k as k_build writes it into the batch planes: [(dot, deps, t_ms)], every dot's seq its rank
        among the segment's dots of its source (seg_rank), deps on the executed prefix dropped."""
        a, b = int(self.start[k]), int(self.end[k])
        dots = self.dot[a:b + 1].astype(np.int64)
        src, seq = dots >> _lib.FX_SEQ_BITS, dots & _lib.FX_SEQ_MASK

        def rank(d):
            same = (src == (d >> _lib.FX_SEQ_BITS)) if by_source else np.ones(len(src), bool)
            return (d >> _lib.FX_SEQ_BITS, 1 + int((same & (seq < (d & _lib.FX_SEQ_MASK))).sum()))

        out = []
        for i in range(a, b + 1):
            deps = [int(self.deps[j][i]) for j in range(int(self.nd[i]))]
            kept = [rank(u) for u, p in zip(deps, self.position(np.array(deps, np.uint32))) if p >= a]
            out.append((rank(int(self.dot[i])), kept, i))
        return out


class Analysis:
    """The batch: streams [StreamCut] and what the driver must report and do (the module docstring)."""

    def __init__(self, planes, no_carry=None, max_seg=MAX_SEG, singles="cut"):
        self.S, self.steps = planes.S, planes.steps
        self.nch = (planes.steps + CHUNK - 1) // CHUNK
        if no_carry == CHUNK * CHUNK and self.nch <= BLK_ABOVE:
            no_carry = None  # k_chunk_excl has no rounds
        self.streams = [StreamCut(planes, s, no_carry, max_seg) for s in range(planes.S)]
        self.scan_kernel = "k_chunk_excl_blk" if self.nch > BLK_ABOVE else "k_chunk_excl"
        self.ptotal = sum(planes.n * (st.max_seq + 1) for st in self.streams)
        self.sparse = self.ptotal > SPARSE_ABOVE
        self.small = planes.S <= SMALL_S  # part + k_part_max, and item() in plane order
        cut = [st for st in self.streams if not st.whole]
        self.whole = [st.s for st in self.streams if st.whole]
        self.whole_streams = len(self.whole)
        self.NS = sum(len(st.end) for st in self.streams)
        self.segments = sum(len(st.end) for st in cut)
        self.max_segment = max([1] + [int(st.length.max()) for st in cut if len(st.length)])
        # classes over every stream: a whole stream's segments keep their (empty) batch slots
        self.class_counts = [0] * NCLS
        for st in self.streams:
            for c, k in zip(*np.unique(st.cls, return_counts=True)):
                self.class_counts[int(c)] += int(k)
        self.slots = sum(self.class_counts[1:])
        self.class_chunks = (self.NS + CHUNK - 1) // CHUNK
        if singles == "cut":
            self.single_segments = sum(st.singles() for st in cut)
        else:  # the driver before: NS - h_nbatch
            self.single_segments = self.NS - self.slots if self.segments else 0
        # a double dot's position is whichever atomicExch came last: reach, and every count over all streams, race
        self.racy = any(DOUBLE_DOT in st.reasons for st in self.streams)
        self.nl = sum(self.class_counts[RANK_CLASS_MIN:])
        self.nl_adds = sum(k << min(c, 12) for c, k in enumerate(self.class_counts) if c >= RANK_CLASS_MIN)
        self.rank_kernel = None
        if self.segments:
            self.rank_kernel = "k_rank_slots" if self.nl_adds * RANK_SLOTS_FACTOR < planes.S * planes.steps else "k_rank"

    def stats(self):
        return dict(segments=self.segments, single_segments=self.single_segments, max_segment=self.max_segment,
                    whole_streams=self.whole_streams)


def analyse(planes, **variant):
    return Analysis(planes, **variant)


def oracle_flags(release, s, L, steps):
    """The cut flags from the oracle's release plane alone: step t is a cut exactly when every Add of steps
    0..t has executed by the end of step t, max(release[0..t]) <= t, FX_RELEASE_NONE counting as infinity."""
    rel = release[_lib.index(np.arange(L), s, steps)].astype(np.int64)
    return np.maximum.accumulate(rel) <= np.arange(L)
