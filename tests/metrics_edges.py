"""Hand-built inputs of the metrics pass (fx_batch_metrics, graph_metrics.hip), one per edge of the kernel, shared
by the CPU and the GPU tests.  No executor runs: a case is the planes hdr, order and release and the counts nexec
as some executor could have left them, or as no executor would (rows that must not count).  Everything the call
must not read holds the byte 0xA5: order rows at or above nexec, the release rows of arrivals no counted row names
(where a case does not set them to FX_RELEASE_NONE), header rows no sample reads, pad rows and pad streams.  The
expected histograms come from the restatement (metrics_ref), whose own answers test_metrics_edges_ref.py pins.

The launch shapes restated from fx_batch_metrics: blocks(), grid(), permuted(), lds_bytes(), uses_lds().
PAIRS: the (nbins_chain, nbins_delay) every case runs at: the smallest legal histograms, a usual size, the last
pair that counts in LDS (exactly LDS_BYTES) and the first that adds to the global histograms directly.

How a stream is built (Case.stream): arrival a releases at its anchor row min(a | 15, steps - 1), whose header
time is BASE; a's own header time is BASE - d for the delay d wanted (d < 0: the release is earlier than the
arrival and the u32 difference wraps); an anchor that is executed releases itself, delay 0.  Header bits 24..31
hold a pattern that differs from row to row."""
import functools

import numpy as np

import metrics_ref
from fantoch_amd import _lib

A5 = 0xA5A5A5A5
STALE = 0x25A5A5A5  # the fill without FX_ORDER_SCC_START: an unflagged row above nexec
FLAG = _lib.FX_ORDER_SCC_START
NONE = _lib.FX_RELEASE_NONE
BASE = 0x800000
T_MAX = 0xFFFFFF

LDS_BYTES = 48 * 1024  # METRICS_LDS_BYTES of fx_metrics.h
NBC = 64
LAST_LDS = (NBC, LDS_BYTES // 4 - NBC)
PAIRS = [(2, 2), (64, 4096), LAST_LDS, (NBC, LAST_LDS[1] + 1)]
MAX_GRID = 256 * 8


def lds_bytes(nbc, nbd):
    return (nbc + nbd) * 4


def uses_lds(nbc, nbd):
    return lds_bytes(nbc, nbd) <= LDS_BYTES


def blocks(S, steps):
    """The 256-thread blocks of work: S <= 64 packs the 4 S used words of every 4-row block, S > 64 takes whole tiles."""
    steps4 = (steps + 3) // 4
    return (4 * S * steps4 + 255) // 256 if S <= 64 else ((S + 63) // 64) * steps4


def grid(S, steps):
    return min(blocks(S, steps), MAX_GRID)


def permuted(S, steps):
    """The launch deals its blocks in the XCD order (narrow batches whose grid is a multiple of 8)."""
    return S <= 64 and grid(S, steps) > 0 and grid(S, steps) % 8 == 0


def start_bins(nbins):
    """Bins that are not zero before the call: 1, 2^32 - 1 and 2^40 in turn."""
    return np.resize(np.array([1, (1 << 32) - 1, 1 << 40], np.uint64), nbins)


class Case:
    def __init__(self, name, S, steps):
        self.name, self.S, self.steps = name, S, steps
        self.plane = _lib.plane_words(S, steps)
        self.hdr, self.order, self.release = (np.full(self.plane, A5, np.uint32) for _ in range(3))
        self.nexec = np.full(S, A5, np.uint32)
        self._samples = None

    def at(self, rows, s):
        return _lib.index(rows, s, self.steps)

    def hi(self, rows, s):
        """Header bits 24..31 of a row: ndeps and kind, nothing the pass may look at."""
        return ((np.asarray(rows, np.int64) * 37 + s * 11 + 1) & 0xFF) << 24

    def stream(self, s, rec, flags, delays):
        """Stream s executed len(rec) rows: order row k is arrival rec[k], flagged where flags[k], with the delay
        delays[k] (an executed anchor: 0)."""
        rec, delays = np.asarray(rec, np.int64), np.asarray(delays, np.int64)
        anchor = np.minimum(rec | 15, self.steps - 1)
        self.hdr[self.at(anchor, s)] = BASE | self.hi(anchor, s)
        t = BASE - np.where(anchor == rec, 0, delays)
        assert np.all((t >= 0) & (t <= T_MAX))
        self.hdr[self.at(rec, s)] = t | self.hi(rec, s)
        self.release[self.at(rec, s)] = anchor
        self.order[self.at(np.arange(len(rec)), s)] = rec | (np.asarray(flags, np.int64) << 31)
        self.nexec[s] = len(rec)

    def samples(self):
        if self._samples is None:
            self._samples = metrics_ref.samples(self.hdr, self.order, self.release, self.nexec, self.S, self.steps)
        return self._samples

    def expected(self, nbc, nbd, chain0=None, delay0=None, calls=1):
        """(chain, delay) after `calls` calls over bins that start at chain0 / delay0 (None: zero)."""
        delays, sizes = self.samples()
        chain, delay = chain0, delay0
        for _ in range(calls):
            chain, delay = metrics_ref.bins(sizes, nbc, chain), metrics_ref.bins(delays, nbd, delay)
        return chain, delay


def flags_of(sizes, rows, lead=0):
    """Flags of `rows` order rows: `lead` rows before the first flag, then SCCs of the sizes."""
    flags = np.zeros(rows, np.int64)
    at = lead
    for size in sizes:
        flags[at] = 1
        at += size
    assert at == rows
    return flags


# delays around every clamp of PAIRS, a wrap (-1) and many small ones
PALETTE = [0, 0, 0, 0, 1, 1, 2, 3, 5, 17, 62, 63, 64, 100, 4094, 4095, 4096, LAST_LDS[1] - 2, LAST_LDS[1] - 1,
           LAST_LDS[1], LAST_LDS[1] + 1, -1]


def random_stream(c, s):
    """A stream that depends on (steps, s) alone: the same on either side of S = 64."""
    rng = np.random.RandomState(c.steps * 1000 + s)
    steps = c.steps
    ne = steps if s % 3 == 0 else int(rng.randint(0, steps + 1))
    rec = rng.permutation(steps)[:ne]
    flags = (rng.rand(ne) < 0.6).astype(np.int64)
    if ne and s % 2 == 0:
        flags[0] = 1
    c.stream(s, rec, flags, rng.choice(PALETTE, ne))
    if s % 4 == 1:  # arrivals that never executed, as an executor marks them
        left = np.setdiff1d(np.arange(steps), rec)
        c.release[c.at(left, s)] = NONE


def shape(kind, S, steps):
    c = Case("%s %dx%d" % (kind, S, steps), S, steps)
    for s in range(S):
        random_stream(c, s)
    return c


SPECIAL = (41, 43)  # delays that only the rows of the last blocks have (stride cases)


def stride(S, steps):
    """Every stream executes every arrival: order row k is arrival (k + rot) % steps with a delay in 0..5, but
    the rows of the blocks from MAX_GRID on (a second pass of the grid-stride loop) name arrivals that are no
    anchors and have the delays SPECIAL: 41 in the even blocks (2048, 2050), 43 in the odd ones, and no other row
    has either, so a block the loop drops empties a bin."""
    assert S >= 64 and blocks(S, steps) > MAX_GRID
    c = Case("stride %dx%d" % (S, steps), S, steps)
    k = np.arange(steps)
    for s in range(S):
        blk = k // 4 if S == 64 else (s // 64) * ((steps + 3) // 4) + k // 4
        late = np.flatnonzero(blk >= MAX_GRID)
        rot = steps - late[0] + 16 * (1 + s % 32) if len(late) else 7 * s + 5
        d = np.where(blk < MAX_GRID, (k + s) % 6, np.where(blk % 2 == 0, SPECIAL[0], SPECIAL[1]))
        c.stream(s, (k + rot) % steps, k % (1 + s % 5) == 0, d)
    return c


def chain_rows():
    """SCCs that start on rows 3, 4, 255 and 256 (stream 0); one from row 3 across the 4-row block and one from
    row 255 across row 256 (stream 1); one from row 255 to the end (stream 2, whose row 255 is the last word of
    a 256-thread block in the narrow mapping: 63 * 12 + 8 + 3 = 767)."""
    c = Case("chain rows 3x260", 3, 260)
    k = np.arange(260)
    c.stream(0, k, flags_of([1, 251, 1, 4], 260, lead=3), k % 3)
    c.stream(1, k, flags_of([3, 5, 247, 2, 3], 260), k % 5)
    c.stream(2, k, flags_of([4, 251, 5], 260), k % 2)
    return c


def uniform(name, S, delay, size):
    """64 rows per stream, row k of stream s with the delay delay(s, k) (a function of s and k % 4) and SCCs of
    size(s) rows.  Arrival 63 is the anchor of all and never executes; order row 63 names arrival 3 again."""
    c = Case(name, S, 64)
    k = np.arange(64)
    rec = np.where(k < 63, k, 3)
    for s in range(S):
        c.hdr[c.at(63, s)] = BASE | c.hi(63, s)
        c.hdr[c.at(rec, s)] = (BASE - delay(s, rec)) | c.hi(rec, s)
        c.release[c.at(rec, s)] = 63
        c.order[c.at(k, s)] = rec | ((k % size(s) == 0).astype(np.int64) << 31)
        c.nexec[s] = 64
    return c


def no_count():
    c = Case("rows that do not count 6x21", 6, 21)
    steps, k = 21, np.arange(21)
    # stream 0: nexec 0, every word the fill
    c.nexec[0] = 0
    c.stream(1, [5], [1], [3])
    random_stream(c, 3)  # s % 3 == 0: nexec == steps
    c.hdr[c.at(k, 2)], c.order[c.at(k, 2)], c.release[c.at(k, 2)] = (
        c.hdr[c.at(k, 3)], c.order[c.at(k, 3)], c.release[c.at(k, 3)])
    c.nexec[2] = c.nexec[3]
    # streams 3 and 4: a row with rec == steps, one with rec == 0x7FFFFFFF, one whose release is NONE, one
    # whose release is `steps` and one whose rec is a row's index with bit 30 set: on flagged rows (the SCCs they start are skipped, rows behind them included) ...
    c.hdr[c.at(k, 3)] = c.order[c.at(k, 3)] = c.release[c.at(k, 3)] = A5
    c.stream(3, k, flags_of([2, 3, 4, 5, 3, 4], steps), k % 4)
    c.order[c.at(2, 3)] = steps | FLAG
    c.order[c.at(5, 3)] = 0x7FFFFFFF | FLAG
    c.release[c.at(9, 3)] = NONE
    c.release[c.at(14, 3)] = steps
    c.order[c.at(17, 3)] = 0x40000000 | 17 | FLAG  # all 31 bits are the record index: no row 17 this
    # ... and on unflagged ones (the SCCs around them keep their sizes, 10 and 11)
    c.stream(4, k, flags_of([10, 11], steps), k % 4)
    c.order[c.at(1, 4)] = steps
    c.order[c.at(3, 4)] = 0x7FFFFFFF
    c.release[c.at(11, 4)] = NONE
    c.release[c.at(13, 4)] = steps
    c.order[c.at(15, 4)] = 0x40000000 | 15
    # stream 5: every row good, but a count of steps + 1 (steps % 4 == 1: row `steps` is a pad row of the plane)
    c.stream(5, k, flags_of([1] * steps, steps), k % 4)
    c.nexec[5] = steps + 1
    return c


def empty(S, steps):
    return Case("empty %dx%d" % (S, steps), S, steps)


@functools.lru_cache(maxsize=None)
def shared_cases():
    """The cases that do not depend on the bin pair."""
    tails = [shape("narrow tails", S, steps) for S, steps in
             ((1, 1), (1, 3), (3, 5), (5, 7), (63, 4), (64, 28), (64, 32), (1, 2048))]
    sides = [shape("narrow / tiled", S, steps) for S, steps in ((64, 40), (65, 40), (129, 9), (130, 9))]
    strides = [stride(64, 8197), stride(65, 4101)]
    by_k = lambda s, a: 4 * (s % 16) + a % 4
    extremes = [uniform("one bin 64x64", 64, lambda s, a: 5 + 0 * a, lambda s: 1),
                uniform("all bins 64x64", 64, lambda s, a: s + 0 * a, lambda s: 1 + s % 7),
                uniform("all bins of a wave 64x64", 64, by_k, lambda s: 1 + s % 7),
                uniform("all bins of a wave 65x64", 65, by_k, lambda s: 1 + s % 7)]
    return tuple(tails + sides + strides + [chain_rows()] + extremes + [no_count(), empty(0, 8), empty(8, 0)])


@functools.lru_cache(maxsize=None)
def clamp_cases(nbc, nbd):
    """The cases built for one bin pair."""
    # delays of exactly nbd - 2, nbd - 1, nbd, 0 and 0xFFFFFF, and two releases earlier than the arrival
    # (-1 and -0xFFFFFF as a u32: the last bin); header bits 24..31 all ones
    d = Case("delay clamp 4x16", 4, 16)
    wanted = [nbd - 2, nbd - 1, nbd, 0, T_MAX]
    for s in range(4):
        t = {15: T_MAX, 14: 1 if s % 2 == 0 else T_MAX}
        t.update({a: T_MAX - want for a, want in enumerate(wanted)})
        rel = {a: 15 for a in range(5)}
        rel.update({15: 15, 14: 4})  # arrival 4 has time 0
        rows = np.roll([0, 1, 2, 3, 4, 14, 15], s)
        ne = 7 if s < 3 else 5  # stream 3 stops early: rows 5 and 6 hold the fill, their arrivals' rows too
        for a in rows[:ne]:
            d.hdr[d.at(a, s)] = t[int(a)] | 0xFF000000
            d.release[d.at(a, s)] = rel[int(a)]
        flags = [[1] * 7, [1] + [0] * 6, [1, 0] * 3 + [1], [1] * 7][s]
        d.order[d.at(np.arange(ne), s)] = rows[:ne] | (np.asarray(flags[:ne], np.int64) << 31)
        d.nexec[s] = ne
    steps = nbc + 6
    k = np.arange(steps)
    # one SCC over the whole stream; rows before the first flag, then nbc + 3 rows from row 3; nbc rows from row 4
    a = Case("chain clamp a 3x(nbc+6)", 3, steps)
    a.stream(0, k, flags_of([steps], steps), k % 3)
    a.stream(1, k, flags_of([nbc + 3], steps, lead=3), k % 3)
    a.stream(2, k, flags_of([4, nbc, 2], steps), k % 3)
    # nbc - 2 rows; nbc - 1 rows behind an unflagged row; an SCC of 5 rows that nexec cuts to 3, the rows above
    # nexec being unflagged words here, so that only the count ends the SCC
    b = Case("chain clamp b 3x(nbc+6)", 3, steps)
    b.stream(0, k, flags_of([z for z in (nbc - 2,) if z > 0] + [1] * (steps - (nbc - 2)), steps), k % 3)
    b.stream(1, k, flags_of([nbc - 1] + [1] * (steps - nbc), steps, lead=1), k % 3)
    b.stream(2, k[:steps - 2], flags_of([1, nbc, 3], steps - 2), k[:steps - 2] % 3)
    b.order[b.at(k[steps - 2:], 2)] = STALE
    return (d, a, b)


def all_cases(nbc, nbd):
    return list(shared_cases()) + list(clamp_cases(nbc, nbd))


NAMES = [c.name for c in all_cases(*PAIRS[0])]
ACCUMULATE = ["narrow tails 5x7", "narrow / tiled 65x40", "delay clamp 4x16", "rows that do not count 6x21"]


def case(name, nbc, nbd):
    return all_cases(nbc, nbd)[NAMES.index(name)]


def params():
    """(case name, nbc, nbd) of every run, and their ids."""
    rows = [(name, nbc, nbd) for nbc, nbd in PAIRS for name in NAMES]
    return rows, ["%s-%dx%d" % (name.replace(" ", "_"), nbc, nbd) for name, nbc, nbd in rows]
