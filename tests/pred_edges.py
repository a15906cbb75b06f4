"""The predecessors executor's edge cases (test infrastructure): hand-built
streams, each the smallest that reaches one place where a table of
fantoch_amd/csrc/pred_exec.hip ends, paired with one that exceeds it by a
single command or a single seq, and the planes the restatement (pred_ref)
expects of a tier over buffers of 0xA5 bytes.  Shared by the CPU tests
(test_pred_edges_ref.py: the pair conditions, the oracle) and the GPU tests
(test_pred_edges_gpu.py).

An Add is (dot, deps, t_ms, (clock seq, clock process id)); t_ms = 9 * row, so
delays pass the ExecutionDelay histogram's last bin where a command waits
more than 455 rows.

What the tables' sizes make unreachable, and so is not a case here:
  * the frame stack outside the compiled n = 5 layout: FD = P there, every
    live frame belongs to a pending command, and the vertices run out first;
  * an execution at exactly seq - frontier - 1 == W on the executed clock.
    The executed frontier f lags the committed one only while (p, f + 1) is
    pending, which holds index slot (f + 1) mod Q, and Q divides W in every
    layout: (p, f + 1 + W) stops at the index.  The exceeding streams commit
    (p, f + 2 + W), two past the last that fits; the seqs that would share
    the stuck dot's index slot are left out of these streams.
"""
import functools
import random

import numpy as np

import metrics_ref
import pred_ref as R
import pred_shapes as PS
from fantoch_amd import _lib
from fantoch_amd import streams as fs

FILL = 0xA5
A5 = 0xA5A5A5A5
SMALL, LDS, HBM = R.SMALL, R.LDS, R.HBM
NAMES = ("order", "release", "nexec", "err")
NEVER = (2, 0xFFFF)  # a dep that no stream here commits


def T(stream):
    """The rows (dot, deps, clock) with their times."""
    return [(d, deps, 9 * i, c) for i, (d, deps, c) in enumerate(stream)]


class Pair:
    """fit / exceed: stream indexes of a case; the exceeding one is stopped at
    `tier` by `resource` (`clock`: which window), the fitting one peaks at the
    limit less `short`."""

    def __init__(self, fit, exceed, resource, tier, short=0, clock=None):
        self.fit, self.exceed, self.resource, self.tier = fit, exceed, resource, tier
        self.short, self.clock = short, clock


class Case:
    def __init__(self, name, n, streams, tiers, dmax=None, pairs=(), hand=None, header_nd=False, long_length=None):
        self.name, self.n, self.streams, self.tiers, self.pairs, self.hand = name, n, streams, tuple(tiers), pairs, hand
        self.header_nd = header_nd  # run without the ndeps plane: FX_HDR_ND counts the deps
        self._dmax, self._long, self._packed, self._restated = dmax, long_length, None, {}

    @property
    def S(self):
        return len(self.streams)

    def packed(self):
        """(planes, clock_lo, clock_hi, ndeps), the deps planes widened to the case's dmax."""
        if self._packed is None:
            planes, clo, chi, nd = PS.pack_pred_streams(self.streams, self.n)
            if self._dmax is not None and self._dmax != planes.dmax:
                assert self._dmax > planes.dmax
                deps = np.zeros(self._dmax * planes.plane, np.uint32)
                deps[:planes.deps.size] = planes.deps
                planes = fs.Planes(planes.S, planes.steps, self._dmax, planes.n, planes.dot, planes.hdr, deps,
                                   planes.lengths)
            if self._long is not None:  # a length above steps: the kernel runs `steps` rows
                assert len(self.streams[self._long]) == planes.steps
                planes.lengths[self._long] = planes.steps + 7
            self._packed = planes, clo, chi, nd
        return self._packed

    @property
    def dmax(self):
        return self.packed()[0].dmax

    def limits(self, tier):
        return None if tier is None else R.tier_limits(tier, self.n, self.dmax)

    def restated(self, s, tier, at_commit=False):
        """pred_ref.run of stream s at a tier's limits (None: unbounded)."""
        key = (s, self.limits(tier), at_commit)
        if key not in self._restated:
            self._restated[key] = R.run(self.streams[s], self.n, self.limits(tier), at_commit)
        return self._restated[key]

    def laddered(self, s, at_commit=False):
        """(result, reruns) of stream s through fx_pred_run's chain."""
        reruns = -1
        for tier in R.chain(self.n, self.dmax):
            r = self.restated(s, tier, at_commit)
            reruns += 1
            if r["err"] != R.FX_ERR_CAPACITY:
                break
        return r, reruns

    def planes_of(self, results):
        """order, release, nexec, err as a launch must leave them over buffers of 0xA5 bytes
        (results: stream -> restated result; the other streams keep the fill)."""
        planes = self.packed()[0]
        pw, steps = planes.plane, planes.steps
        order, release = np.full(pw, A5, np.uint32), np.full(pw, A5, np.uint32)
        nexec, err = np.full(self.S, A5, np.uint32), np.full(self.S, A5, np.uint32)
        for s, r in results.items():
            if r["order"]:
                order[_lib.index(np.arange(r["nexec"]), s, steps)] = \
                    np.asarray(r["order"], np.uint32) | np.uint32(R.SCC_START)
                rows = np.fromiter(r["release"].keys(), np.int64)
                release[_lib.index(rows, s, steps)] = np.fromiter(r["release"].values(), np.uint32)
            nexec[s], err[s] = r["nexec"], r["err"]
        return dict(order=order, release=release, nexec=nexec, err=err)

    def expected(self, tier, at_commit=False, only=None):
        return self.planes_of({s: self.restated(s, tier, at_commit) for s in range(self.S)
                               if only is None or s in only})

    def expected_ladder(self, at_commit=False):
        """(planes, reruns, status) fx_pred_run must leave."""
        runs = [self.laddered(s, at_commit) for s in range(self.S)]
        errs = [r["err"] for r, _ in runs if r["err"]]
        return self.planes_of({s: r for s, (r, _) in enumerate(runs)}), sum(k for _, k in runs), errs[0] if errs else 0

    def check(self, res, want):
        for name in NAMES:
            a, b = getattr(res, name), want[name]
            assert np.array_equal(a, b), "%s: %s differs at word %d" % (self.name, name, int(np.flatnonzero(a != b)[0]))


def delay_hist(planes, order, release, nexec, nbins, streams=None):
    """The ExecutionDelay histogram fx_batch_metrics (graph_metrics.hip) must give: per executed command the
    header time of its releasing step less that of its arrival, the last bin taking everything from nbins - 1 up."""
    streams = range(planes.S) if streams is None else streams
    for s in streams:
        k = int(nexec[s])
        rec = (order[_lib.index(np.arange(k), s, planes.steps)] & np.uint32(0x7FFFFFFF)).astype(np.int64)
        assert np.all(release[_lib.index(rec, s, planes.steps)].astype(np.int64) < planes.steps)
    return metrics_ref.hists(planes.hdr, order, release, nexec, planes.S, planes.steps, 2, nbins, streams)[1]


def spread(i, n):
    """The i-th dot (from 0) dealt over n sources."""
    return (1 + i % n, 1 + i // n)


def tier_n(tier):
    """(n, dmax) that select a tier's layout for the cases that do not care: `5` names the compiled SMALL layout."""
    return (5, 5) if tier == 5 else (2, None)


def tier_of(key):
    return SMALL if key == 5 else key


def lim_of(key, dmax=1):
    n, d = tier_n(key)
    return R.tier_limits(tier_of(key), n, d or dmax)


# ------------------------------------------------------------------ vertices
def vertices_stream(K, n):
    """K commands waiting on one dot, then that dot with the lowest clock: K + 1 pending, one list of K."""
    last = (n, 40)
    rows = [(spread(i, n - 1) if n > 2 else (1, i + 1), [last], (i + 2, 1)) for i in range(K)]
    return T(rows + [(last, [], (1, 2))])


def vertices(key):
    n, dmax = tier_n(key)
    P = lim_of(key).P
    return Case("vertices %s" % key_name(key), n, [vertices_stream(P - 1, n), vertices_stream(P, n)], [tier_of(key)],
                dmax, [Pair(0, 1, "vertices", tier_of(key))])


def vertices_hbm():
    """Each waiter waits on a dot of its own that never commits: no list is long (the rank sort is quadratic in
    a list).  The fitting stream ends with everything pending."""
    P = lim_of(HBM).P
    st = lambda K: T([((1, i + 1), [(2, i + 1)], (i + 1, 1)) for i in range(K)])
    return Case("vertices HBM", 2, [st(P), st(P + 1)], [HBM], None, [Pair(0, 1, "vertices", HBM)])


# ------------------------------------------------------------------ index
def index(key):
    n, dmax = tier_n(key)
    Q = lim_of(key).Q
    wait, free = [(2, 9)], []
    streams = [
        T([((1, 1), wait, (1, 1)), ((1, Q), free, (2, 1))]),            # the last seq that shares no slot
        T([((1, 1), wait, (1, 1)), ((1, 1 + Q), free, (2, 1))]),        # the slot of a pending dot
        T([((1, 1), free, (1, 1)), ((1, 1 + Q), wait, (2, 1))]),        # a slot freed by execution
        T([((1, 1), wait, (1, 1)), ((2, 1 + Q), free, (2, 1)), ((1, 1 + 2 * Q), free, (3, 1))]),  # per source; 2 turns
    ]
    return Case("index %s" % key_name(key), n, streams, [tier_of(key)], dmax, [Pair(0, 1, "index", tier_of(key))])


# ------------------------------------------------------------------ committed window and ring wrap
def ring_walk(W, shift=0):
    rows = []
    for k in range(1, W):
        rows += [((1, k + W - 1 + shift), [], (2 * k, 1)), ((1, k + shift), [], (2 * k + 1, 1))]
    return T(rows)


def window(key):
    """For k = 1 .. W - 1: (1, k + W - 1), at the window's last position and on the ring bit of the seq the
    frontier has just passed, then (1, k); the last pair walks the frontier through W - 1 set bits.  Shifted up
    by one seq it stops at row 0."""
    n, dmax = tier_n(key)
    W = lim_of(key).W
    return Case("window %s" % key_name(key), n, [ring_walk(W), ring_walk(W, 1)], [tier_of(key)], dmax,
                [Pair(0, 1, "window", tier_of(key), clock="committed")])


def window_hbm():
    W = lim_of(HBM).W
    return Case("window HBM", 2, [T([((1, W), [], (1, 1))]), T([((1, W + 1), [], (1, 1))])], [HBM], None,
                [Pair(0, 1, "window", HBM, clock="committed")])


# ------------------------------------------------------------------ executed window behind a stuck frontier
def stuck_stream(W, Q, last):
    """(1, 1) pends for good; (1, 2) .. (1, W) commit and execute at once (but the seqs on (1, 1)'s index slot);
    then deps inside the ring region of both clocks; then (1, last)."""
    rows = [((1, 1), [NEVER], (1, 1))]
    rows += [((1, s), [], (s, 1)) for s in range(2, W + 1) if s % Q != 1]
    rows += [((2, 1), [(1, 3), (1, Q + 5), (1, W)], (W + 1, 1)),  # committed and executed, by ring bits: executes
             ((2, 2), [(1, Q + 1), (1, 4)], (W + 2, 1)),          # (1, Q + 1) is in the committed ring, not set: waits
             ((2, 3), [(1, 1), (2, 2)], (W + 3, 1))]              # both pending, lower clocks: waits in phase two
    if last:
        rows.append(((1, last), [], (W + 4, 1)))
    return T(rows)


def stuck(key):
    n, dmax = tier_n(key)
    lim = lim_of(key, 3)
    W, Q = lim.W, lim.Q
    assert W % Q == 0
    return Case("stuck frontier %s" % key_name(key), n, [stuck_stream(W, Q, 0), stuck_stream(W, Q, W + 2)],
                [tier_of(key)], dmax, [Pair(0, 1, "window", tier_of(key), clock="executed")])


# ------------------------------------------------------------------ frames (the compiled layout only)
def chain_rows(dots, clock0):
    """c_i depends on c_(i-1), clocks ascend, commits run the last first."""
    rows = [(d, [dots[i - 1]] if i else [], (clock0 + i, 1)) for i, d in enumerate(dots)]
    return rows[::-1]


def frames():
    FD = lim_of(5).FD
    st = lambda K: T(chain_rows([spread(i, 5) for i in range(K)], 1))
    return Case("frames compiled", 5, [st(FD + 1), st(FD + 2)], [SMALL], 5, [Pair(0, 1, "frames", SMALL)])


# ------------------------------------------------------------------ lists
def lists_stream(k, m):
    """z, lowest in clock, stuck; m dummies on z and every x; the chain x_k .. x_1: when x_1 executes the
    recursion holds k lists of a chain link and the m dummies, the last of the dummies alone."""
    z, xs = (2, 1), [(1, i + 1) for i in range(k)]
    rows = [(z, [NEVER], (1, 2))]
    rows += [((2, 2 + j), [z] + xs, (1000 + j, 1)) for j in range(m)]
    return T(rows + chain_rows(xs, 2))


def lists():
    LL = lim_of(SMALL, 17).LL
    k = 16
    m = (LL + 1) // k - 1
    assert k * (m + 1) - 1 == LL - 1
    return Case("lists SMALL", 2, [lists_stream(k, m), lists_stream(k, m + 1)], [SMALL], None,
                [Pair(0, 1, "lists", SMALL, short=1)])


def lists5_stream(groups, extra):
    """The compiled layout: dmax = 5 caps a dummy's deps, so the dummies go by groups of five consecutive links
    of a chain (groups[g] of them on z and links 5g .. 5g + 3; extra: on z and the first nx links)."""
    k = 5 * len(groups)
    z, xs = (5, 30), [spread(i, 4) for i in range(k)]
    rows, j = [(z, [(5, 31)], (1, 2))], 0
    for g, cnt in enumerate(groups):
        for _ in range(cnt):
            rows.append(((5, 1 + j), [z] + xs[5 * g:5 * g + 4], (1000 + j, 1)))
            j += 1
    for nx in extra:
        rows.append(((5, 1 + j), [z] + xs[:nx], (1000 + j, 1)))
        j += 1
    return T(rows + chain_rows(xs, 2))


@functools.lru_cache(None)
def lists5_pair():
    """Dummies added one at a time, group after group, until the restatement reports the stop; then the last
    one's deps trimmed so that the fitting stream ends exactly on the limit where a count allows it."""
    lim = lim_of(5)
    groups, g = [2] * 5, 0
    while True:
        trial = list(groups)
        trial[g % 5] += 1
        if R.run(lists5_stream(trial, ()), 5, lim)["err"]:
            break
        groups, g = trial, g + 1
    best = (R.run(lists5_stream(groups, ()), 5, lim)["peak"]["lists"], ())
    for nx in range(1, 5):
        r = R.run(lists5_stream(groups, (nx,)), 5, lim)
        if not r["err"] and r["peak"]["lists"] > best[0]:
            best = (r["peak"]["lists"], (nx,))
    fit = lists5_stream(groups, best[1])
    exceed = lists5_stream(groups, best[1] + (1,))
    return fit, exceed, lim.LL - best[0]


def lists5():
    fit, exceed, short = lists5_pair()
    return Case("lists compiled", 5, [fit, exceed], [SMALL], 5, [Pair(0, 1, "lists", SMALL, short=short)])


# ------------------------------------------------------------------ clocks
# (clock of a, clock of b, which executes first), a = (1, 1) and b = (2, 1) depending on each other: the one
# with the lower clock (seq, process id) runs first whichever arrives first; equal clocks (no Caesar run has
# them; the compare is strict) hold nobody back, so the earlier arrival, released by the later one's commit,
# runs first.
CLOCK_PAIRS = [
    ((1 << 24, 5), (0, 5), "b"),                        # equal clock_lo, clock_hi 1 and 0
    ((0, 5), (1 << 24, 5), "a"),
    ((1 << 24, 1), (9, 200), "b"),                      # clock_lo order opposite to the full order
    ((9, 200), (1 << 24, 1), "a"),
    ((7, 1), (7, 2), "a"),                              # equal seq, process ids both ways round
    ((7, 2), (7, 1), "b"),
    ((0xFFFFFF, 0xFF), (0x1000000, 0), "a"),            # packed 2^32 - 1 and 2^32
    ((0x1000000, 0), (0xFFFFFF, 0xFF), "b"),
    (((1 << 48) - 1, 0xFF), ((1 << 48) - 1, 0xFE), "b"),  # packed 2^56 - 1 and 2^56 - 2
    (((1 << 48) - 1, 0xFE), ((1 << 48) - 1, 0xFF), "a"),
    (((1 << 48) - 1, 0xFF), ((1 << 47), 0xFF), "b"),    # 2^56 - 1 against a lower clock_hi with the same clock_lo byte
    ((3, 1), (3, 1), "first"),                          # equal: strict, so nobody waits
    (((1 << 48) - 1, 0xFF), ((1 << 48) - 1, 0xFF), "first"),
]


def clocks():
    """Every pair in both arrival orders; hand[s] = the order (arrival indexes) written out by hand."""
    a, b = (1, 1), (2, 1)
    streams, hand = [], []
    for ca, cb, first in CLOCK_PAIRS:
        streams.append(T([(a, [b], ca), (b, [a], cb)]))       # a arrives first: a is arrival 0
        hand.append({"a": [0, 1], "b": [1, 0], "first": [0, 1]}[first])
        streams.append(T([(b, [a], cb), (a, [b], ca)]))       # b arrives first: b is arrival 0
        hand.append({"a": [1, 0], "b": [0, 1], "first": [0, 1]}[first])
    return Case("clocks", 2, streams, [SMALL, LDS, HBM], hand=hand)


def clocks5():
    c = clocks()
    return Case("clocks compiled", 5, c.streams, [SMALL], 5, hand=c.hand)


# ------------------------------------------------------------------ deps count
NDS = (0, 1, 11, 12, 13, 31, 32, 33, 63, 64, 65, 255, 256)


def deps_stream(nd, rank, n=4):
    """A command with nd deps: nd - 1 executed earlier, the one of rank `rank` (ascending by dot) a blocker that
    commits later with a lower clock and waits itself (so the bit is registered in the phase-one index, then in
    the phase-two index), then is released."""
    pool = sorted(spread(i, n) for i in range(nd))
    target, unblock = (n, 100), (n, 101)
    rows = [(d, [], (10 + i, 1)) for i, d in enumerate(pool) if i != rank]
    rows.append((target, pool, (5000, 1)))
    if nd:
        rows += [(pool[rank], [unblock], (2, 1)), (unblock, [], (1, 1))]
    return T(rows)


def deps_ranks(nd):
    return sorted(set(r for r in (0, nd - 1, 31, 32, 63, 64) if 0 <= r < nd)) or [0]


def deps_count():
    streams = [deps_stream(nd, r) for nd in NDS for r in deps_ranks(nd)]
    return Case("deps count", 4, streams, [SMALL, LDS, HBM])


def deps_header():
    """nd <= 31 counted by the header alone (no ndeps plane)."""
    streams = [deps_stream(nd, r) for nd in NDS if nd <= 31 for r in deps_ranks(nd)]
    return Case("deps header", 4, streams, [SMALL, LDS], header_nd=True)


# ------------------------------------------------------------------ lengths and lanes
def mixed_rows(seed, L, n, maxdeps):
    """A seeded stream of L Adds over n sources: deps among nearby dots, a few never committed."""
    rng = random.Random(seed)
    dots = [spread(i, n) for i in range(L + 4)]
    clock = list(range(1, L + 5))
    rng.shuffle(clock)
    order = sorted(range(L + 4), key=lambda i: i + rng.random() * 6)[:L]
    rows = []
    for i in order:
        near = [j for j in range(max(0, i - 5), min(L + 4, i + 6)) if j != i]
        deps = rng.sample(near, min(len(near), rng.randrange(0, maxdeps + 1)))
        rows.append((dots[i], [dots[j] for j in deps], (clock[i], 1 + i % 3)))
    return rows


def mixed(seed, L, n, maxdeps):
    return T(mixed_rows(seed, L, n, maxdeps))


LENGTHS = (0, 1, 3, 4, 5, 8, 9)


def lengths():
    """The prefetch's edges (a row of 4 steps, loaded one row ahead while r + 4 < len), and a `lengths` entry
    above steps on the longest stream."""
    streams = [mixed(40 + L, L, 3, 4) for L in LENGTHS] + [mixed(60 + L, L, 3, 4) for L in LENGTHS[::-1]]
    return Case("lengths", 3, streams, [SMALL, LDS, HBM], long_length=len(LENGTHS) - 1)


def lengths5():
    streams = [mixed(80 + L, L, 5, 5) for L in LENGTHS] + [mixed(90 + L, L, 5, 5) for L in LENGTHS[::-1]]
    return Case("lengths compiled", 5, streams, [SMALL], 5, long_length=len(LENGTHS) - 1)


def lanes5(S):
    """The compiled layout runs FX_PRED_WPB = 4 streams per workgroup: S streams leave part of the last one empty."""
    return Case("lanes compiled %d" % S, 5, [mixed(7 * s + S, (5 * s + 2) % 14, 5, 5) for s in range(S)], [SMALL], 5)


def many():
    """257 short streams: the XCD slot permutation of a launch of 256 or more is on."""
    return Case("many", 3, [mixed(300 + s, (3 * s + 1) % 11, 3, 3) for s in range(257)], [SMALL, LDS])


# ------------------------------------------------------------------ errors
def errors():
    ok = lambda s, i: ((1, s), [(2, s)], (i + 1, 1))
    streams = [
        T([((0, 1), [], (1, 1)), ok(1, 1)]),                               # source 0 at row 0
        T([((3, 1), [], (1, 1)), ok(1, 1)]),                               # source n + 1 at row 0
        T([((1, 0), [], (1, 1)), ok(1, 1)]),                               # seq 0 at row 0
        T([ok(1, 0), ((2, 1), [], (9, 1)), ((0, 1), [], (3, 1)), ok(2, 3)]),   # the same at a middle row
        T([ok(1, 0), ((2, 1), [], (9, 1)), ((3, 1), [], (3, 1)), ok(2, 3)]),
        T([ok(1, 0), ((2, 1), [], (9, 1)), ((2, 0), [], (3, 1)), ok(2, 3)]),
        T([ok(1, 0), ((2, 0), [], (2, 1)), ok(1, 2), ok(3, 3)]),           # two bad rows: the earlier one wins
        T([ok(1, 0), ok(1, 1), ((2, 0), [], (3, 1))]),                     # a repeat, then a bad dot: the repeat
        T([ok(1, 0), ok(2, 1), ok(1, 2), ((2, 1), [], (9, 1))]),           # a second commit of a pending dot
        T([ok(1, 0), ((2, 1), [], (9, 1)), ((1, 1), [], (3, 1)), ok(2, 3)]),   # and of an executed one
        T([((2, 1), [], (1, 1)), ((2, 3), [], (2, 1)), ((2, 3), [], (3, 1))]),  # and of one above the frontier
    ]
    return Case("errors", 2, streams, [SMALL, LDS, HBM])


def errors5():
    return Case("errors compiled", 5, [[(d if d[0] != 3 else (6, d[1]), deps, t, c) for d, deps, t, c in st]
                                       for st in errors().streams], [SMALL], 5)


def tile_error():
    """One failing stream in a full tile of 64."""
    rows = [mixed_rows(500 + s, 6 + s % 5, 2, 3) for s in range(64)]
    rows[37].insert(3, ((1, 0), [], (1, 1)))
    streams = [T(r) for r in rows]
    return Case("tile error", 2, streams, [SMALL])


def key_name(key):
    return "compiled" if key == 5 else R.TIER_NAME[key]


@functools.lru_cache(None)
def all_cases():
    cases = [vertices(SMALL), vertices(5), vertices(LDS), vertices_hbm()]
    cases += [index(k) for k in (SMALL, 5, LDS, HBM)]
    cases += [window(5), window(SMALL), window(LDS), window_hbm()]
    cases += [stuck(5), stuck(SMALL), stuck(LDS)]
    cases += [frames(), lists(), lists5(), clocks(), clocks5(), deps_count(), deps_header(), lengths(), lengths5()]
    cases += [lanes5(S) for S in (1, 3, 5, 41)]
    cases += [many(), errors(), errors5(), tile_error()]
    return cases
