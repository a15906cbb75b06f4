"""The graph executor's edge cases (test infrastructure): hand-built streams,
each the smallest that reaches one place where a table of a tier of
fantoch_amd/csrc/graph_*.hip ends, paired with one that passes it by a single
Add, and the bytes a launch must leave over buffers of 0xA5.  Shared by the
CPU tests (test_graph_edges_ref.py: the pair conditions, the oracle) and the
GPU tests (test_graph_edges_gpu.py).

An Add is (dot, deps, t_ms) with t_ms = its row.  Sources 1 .. n - 1 carry
the commands under test, dealt round (spread), source n the dots they wait on.

What the tables' sizes make unreachable, and so is no case here:
  * the check_pending worklist's limit, at every tier.  The worklist is emptied
    at the start of a step, and an entry is a dot executed in that step.  An
    executed dot held a vertex when the step's search began, the fast path's
    dot excepted, which is entry 0 and is popped before anything else is
    pushed.  So a step pushes at most as many entries as vertices are held:
    P, and the capacities are P + 1 (GROUP, WAVE, the slot tiers), P + 2
    (LANE_REG, which moreover pushes only dots with waiters) and P / 2 P (the
    wide tiers).  The `worklist` cases release the largest cascades the slots
    hold -- one SCC of P vertices, and P vertices waiting on one dot -- and
    test_graph_edges_ref.py checks that their high-water marks are P (the SCC
    is pushed at once; the waiters one by one while try_pending goes through
    them, the arrived dot popped before);
  * more than C cached deps at LANE_REG: it caches LANE_MAX_DEPS = 8 deps and
    launch_lane refuses a wider batch (graph_lane.hip:828), so the Add with
    C + 1 deps goes to FX_TIER_LDS_LARGE by the routing rule instead;
  * window_bits executed exceptions above a stuck frontier: bit 0 of a window
    is the frontier's own successor, whose execution moves the frontier.  The
    most a window holds is window_bits - 1 exceptions, offsets 1 ..
    window_bits - 1; offset window_bits is the first to stop a stream;
  * the wide tiers' PW and nml: FX_FLAG_PARTIAL only (graph_ref's docstring);
  * a cascade through FX_TIER_WIDE_HBM's full table: releasing 16384 waiters
    of one dot rank-sorts them with 16384 ^ 2 / 64 dependent dot reads from
    HBM in one wavefront, and collects them with 256 passes a popped dot.  Its
    16384 vertices are filled by commands that each wait on a dot of their own
    instead (slots_apart), and its 32768-bit window is walked as the LDS wide
    tier's is (window_late); both are also cut for resume where they are full.
    The reuse and worklist shapes run there at the LDS wide tier's sizes, where
    everything fits (the code is one template, graph_wide.hip:109).

The ladder (fx_batch_run_tiered) starts every batch of at most 16 streams at
each of the nine tiers.  The placement batches and the split batch (63 to 130
streams) start at the tier they are written for only: they are about where a
stopping stream sits in that tier's own launch, and the reruns they cause go
through the same compacted stream map whatever tier came first, which the
small batches already take through every chain.
"""
import functools
import random

import numpy as np

import graph_ref as R
from fantoch_amd import _lib
from fantoch_amd import streams as fs
from oracle import oracle_lib

FILL = 0xA5
A5 = 0xA5A5A5A5
NAMES = ("order", "release", "nexec", "err")
N = 5
GROUP, LDS_LARGE, GLOBAL, LANE, WAVE, LANE_REG, SPLIT, WIDE, WIDE_HBM = range(9)
LIMITED = (GROUP, LDS_LARGE, GLOBAL, LANE, WAVE, LANE_REG, WIDE)  # the tiers taken to their limits
# FX_TIER_SPLIT's rule (graph_split.hip:42-66, fx_internal.h:124): a 64-stream tile whose mean deps per Add, x 8,
# over its first 256 rows is at least 16 runs on the group tier, the others on the lane-register tier
SPLIT_SAMPLE, SPLIT_THRESHOLD = 256, 16


def T(rows):
    return [(d, sorted(deps), i) for i, (d, deps) in enumerate(rows)]


def spread(i, n=N):
    """The i-th dot (from 0) dealt over sources 1 .. n - 1."""
    return (1 + i % (n - 1), 1 + i // (n - 1))


class Pair:
    """fit / exceed: stream indexes; the exceeding one is stopped at `tier` by `resource` at row `row`, its counter
    `counter` one over `limit`, which the fitting one reaches exactly."""

    def __init__(self, fit, exceed, resource, tier, row, counter, limit):
        self.fit, self.exceed, self.resource, self.tier = fit, exceed, resource, tier
        self.row, self.counter, self.limit = row, counter, limit


class Case:
    def __init__(self, name, streams, tiers, pairs=(), n=N, dmax=None):
        self.name, self.n, self.streams, self.tiers, self.pairs = name, n, streams, tuple(tiers), tuple(pairs)
        self._dmax, self._packed, self._oracle, self._restated = dmax, None, None, {}

    @property
    def S(self):
        return len(self.streams)

    def packed(self):
        """The batch's planes, the dep planes widened to the case's dmax."""
        if self._packed is None:
            p = fs.pack_streams(self.streams, self.n)
            if self._dmax is not None and self._dmax != p.dmax:
                assert self._dmax > p.dmax
                deps = np.zeros(self._dmax * p.plane, np.uint32)
                deps[:p.deps.size] = p.deps
                p = fs.Planes(p.S, p.steps, self._dmax, p.n, p.dot, p.hdr, deps, p.lengths)
            self._packed = p
        return self._packed

    @property
    def dmax(self):
        return self.packed().dmax

    def oracle(self):
        """(order, release, nexec, err, max_pending, max_window) of the C++ oracle, computed once."""
        if self._oracle is None:
            self._oracle = oracle_lib.batch_execute(self.packed(), threads=8, stats=True)
            for a in self._oracle:
                a.setflags(write=False)
        return self._oracle

    def restated(self, s, tier=None):
        """graph_ref.run of stream s at a tier's limits (None: unbounded)."""
        if (s, tier) not in self._restated:
            lim = None if tier is None else R.tier_limits(tier, self.n)
            self._restated[(s, tier)] = R.run(self.streams[s], self.n, lim)
        return self._restated[(s, tier)]

    # ---------------------------------------------------------- which tier a stream runs on
    def tile_tier(self, s):
        """The tier FX_TIER_SPLIT runs stream s's tile on."""
        if self.dmax > R.MAX_DEPS[LANE_REG]:
            return GROUP  # launch_split's lane_ok (graph_split.hip:194)
        nd = cnt = 0
        for st in self.streams[64 * (s // 64):64 * (s // 64) + 64]:
            rows = st[:SPLIT_SAMPLE]
            nd += sum(len(set(a[1])) for a in rows)
            cnt += len(rows)
        return GROUP if min(nd * 8 // max(cnt, 1), 63) >= SPLIT_THRESHOLD else LANE_REG

    def fits(self, s, tier):
        if tier == SPLIT:
            tier = self.tile_tier(s)
        return R.fits(self.restated(s)["stats"], tier, self.n)

    def chain(self, first):
        """The tiers fx_batch_run_tiered tries from `first` on (graph_tiers.hip:167-178)."""
        if self.dmax > R.MAX_DEPS[first]:
            first = LDS_LARGE
        out = []
        while first is not None:
            out.append(first)
            first = R.NEXT[first]
        return out

    def tier_counts(self, first):
        """tier_counts of fx_batch_run_tiered: the streams each tier of the chain was given."""
        counts, left = [0] * _lib.FX_NUM_TIERS, list(range(self.S))
        for tier in self.chain(first):
            if not left:
                break
            counts[tier] = len(left)
            left = [s for s in left if not self.fits(s, tier)]
        assert not left, "%s: streams %s fit no tier" % (self.name, left)
        return counts

    # ---------------------------------------------------------- the bytes a launch must leave
    def blank(self):
        p = self.packed()
        return dict(order=np.full(p.plane, A5, np.uint32), release=np.full(p.plane, A5, np.uint32),
                    nexec=np.full(p.S, A5, np.uint32), err=np.full(p.S, A5, np.uint32))

    def put_oracle(self, want, s):
        """Stream s as the oracle has it: its executed rows of order, the release rows of its Adds, nexec, err."""
        p = self.packed()
        order, release, nexec, err = self.oracle()[:4]
        rows = _lib.index(np.arange(int(nexec[s])), s, p.steps)
        want["order"][rows] = order[rows]
        rows = _lib.index(np.arange(len(self.streams[s])), s, p.steps)
        want["release"][rows] = release[rows]
        want["nexec"][s], want["err"][s] = nexec[s], err[s]

    def expected_ladder(self):
        want = self.blank()
        for s in range(self.S):
            self.put_oracle(want, s)
        return want

    def check_launch(self, res, tier, streams=None):
        """One launch at `tier` over buffers of 0xA5 (streams: the launch's stream_map, None: all).  A stream that
        fits the tier equals the oracle in every byte; one that the tier stops has err == FX_ERR_CAPACITY and is
        checked by check_stopped; every other byte of the four outputs is 0xA5."""
        p = self.packed()
        want = self.blank()
        own = np.zeros(p.plane, bool)  # rows of stopped streams, checked apart
        for s in range(self.S) if streams is None else streams:
            run_tier = self.tile_tier(s) if tier == SPLIT else tier
            r = self.restated(s, run_tier)
            if r["err"] == 0:
                assert self.oracle()[3][s] == 0
                self.put_oracle(want, s)
            else:
                assert r["err"] == _lib.FX_ERR_CAPACITY
                want["err"][s] = _lib.FX_ERR_CAPACITY
                want["nexec"][s] = res.nexec[s]
                own[_lib.index(np.arange(r["row"] + 1), s, p.steps)] = True
                self.check_stopped(res, s, r["row"])
        for name in ("nexec", "err"):
            a, b = getattr(res, name), want[name]
            assert np.array_equal(a, b), "%s: %s differs at stream %d" % (
                self.name, name, int(np.flatnonzero(a != b)[0]))
        for name in ("order", "release"):
            a, b = getattr(res, name)[~own], want[name][~own]
            assert np.array_equal(a, b), "%s: %s differs at word %d" % (
                self.name, name, int(np.flatnonzero(~own)[np.flatnonzero(a != b)[0]]))

    def check_stopped(self, res, s, row):
        """A stream its tier stopped at `row`.  Defined, at every tier: nexec counts at least what executed before
        that step and at most what executes in it too, and order below nexec is the oracle's; release of an Add
        before `row` is the oracle's step if that is before `row`, FX_RELEASE_NONE if it is later or never.
        Left open: an Add released in the stopping step itself holds that step or FX_RELEASE_NONE (LANE_REG
        drops an SCC from its table only when all of it is out, so a stop inside one reports the members it has
        already written as pending; the others leave the step in place), and the stopping row holds either of
        those or the fill (the slot tiers take the slot before they count the deps, LANE_REG writes a row's block
        from registers).  Rows past `row`, and order from nexec on, keep the fill: check_launch compares them."""
        p = self.packed()
        order, release, nexec = self.oracle()[:3]
        k = int(nexec[s])
        rec = (order[_lib.index(np.arange(k), s, p.steps)] & np.uint32(0x7FFFFFFF)).astype(np.int64)
        steps = release[_lib.index(rec, s, p.steps)].astype(np.int64)
        assert np.all(np.diff(steps) >= 0)
        lo, hi = int((steps < row).sum()), int((steps <= row).sum())
        got = int(res.nexec[s])
        assert lo <= got <= hi, "%s stream %d: nexec %d outside [%d, %d]" % (self.name, s, got, lo, hi)
        rows = _lib.index(np.arange(p.steps), s, p.steps)
        assert np.array_equal(res.order[rows[:got]], order[rows[:got]]), "%s stream %d: order" % (self.name, s)
        assert np.all(res.order[rows[got:]] == A5), "%s stream %d: order past nexec" % (self.name, s)
        for a in range(row + 1):
            want, have = int(release[rows[a]]), int(res.release[rows[a]])
            if a == row:
                ok = have in (row, R.FX_RELEASE_NONE, A5)
            elif want < row:
                ok = have == want
            elif want == row:
                ok = have in (row, R.FX_RELEASE_NONE)
            else:
                ok = have == R.FX_RELEASE_NONE
            assert ok, "%s stream %d: release[%d] = %#x, the oracle has %#x" % (self.name, s, a, have, want)


def slots_held(lim):
    """Vertices that may wait while one more Add arrives: the wide tiers give that Add a vertex too."""
    return lim.P - 1 if lim.wide else lim.P


# ------------------------------------------------------------------ slots
def waiting(K, on, n=N):
    return [(spread(i, n), [on]) for i in range(K)]


def slots(tier, n=N):
    """K commands wait on one dot, which then arrives: K + 1 of them stop the tier at the last one's row (at the
    wide tiers, which give the arriving dot a vertex as well, at that dot's row)."""
    lim = R.tier_limits(tier, n)
    K, b = slots_held(lim), (n, 1)
    fit = T(waiting(K, b, n) + [(b, [])])
    exceed = T(waiting(K + 1, b, n) + [(b, [])])
    return Case("slots %s n=%d" % (R.TIER_NAME[tier], n), [fit, exceed], [tier],
                [Pair(0, 1, "slots", tier, K + 1 if lim.wide else K, "slots_all" if lim.wide else "slots", lim.P)], n)


def slots_reuse(tier):
    """The table full, one command executes, another arrives into the freed slot; in the twin the dot that would
    have released one is another dot."""
    lim = R.tier_limits(tier, N)
    K, b, b2 = slots_held(lim), (N, 1), (N, 2)
    head = [(spread(0), [b2])] + [(spread(i), [b]) for i in range(1, K)]
    tail = [(spread(K), [b]), (b, [])]
    fit = T(head + [(b2, [])] + tail)
    exceed = T(head + [((N, 3), [])] + tail)
    return Case("slots reuse %s" % R.TIER_NAME[tier], [fit, exceed], [tier],
                [Pair(0, 1, "slots", tier, K + 2 if lim.wide else K + 1, "slots_all" if lim.wide else "slots", lim.P)])


# ------------------------------------------------------------------ cached deps
def cache(tier):
    """A command with exactly C deps not yet executed, which then arrive one by one (the command is registered on
    each in turn); with a dep more, one that never arrives, the tier stops at row 0."""
    C = R.CACHE[tier]
    st = lambda k: T([((1, 1), [(2, j + 1) for j in range(k)])] + [((2, j + 1), []) for j in range(C)])
    return Case("cache %s" % R.TIER_NAME[tier], [st(C), st(C + 1)], [tier], [Pair(0, 1, "cache", tier, 0, "cache", C)])


def widest(tier):
    """An Add as wide as the tier reads (max_deps: the routing rule must leave it there) of whose deps more than C
    are executed already and the rest, at most C, are not: only those count."""
    D, C = R.MAX_DEPS[tier], R.CACHE[tier]
    ex = max(C + 1, D - C) if C is not None and D > C else D // 2
    done = [(1 + j % 2, 1 + j // 2) for j in range(ex)]
    late = [(3, j + 1) for j in range(D - ex)]
    rows = [(d, []) for d in sorted(done)] + [((4, 1), done + late)] + [(d, []) for d in late] + [((4, 2), [(4, 1)])]
    return Case("widest %s" % R.TIER_NAME[tier], [T(rows), T(rows[:ex + 1])], [tier], dmax=D)


# ------------------------------------------------------------------ executed-clock window
def stuck_head(held):
    """What keeps source 1's frontier at 0, and what then moves it.  held: (1, 1) is pending, on (N, 1), which
    arrives to release it.  Not held: (1, 1) itself is late.  The LDS wide tier takes the second form: its
    index gives (1, 1) and (1, 257) one slot, so under a pending (1, 1) the seqs 257, 513, 769 and 1025 -- the
    very seq one past its 1024-bit window -- would stop the stream at the index, not at the window."""
    return ([((1, 1), [(N, 1)])], ((N, 1), [])) if held else ([], ((1, 1), []))


def stuck(W, extra, release=True, held=True, after=False):
    """Source 1's frontier stays 0 (stuck_head) while (1, 2) .. (1, W) execute above it, offsets 1 .. W - 1
    (extra: and (1, W + 1), offset W, the one Add the exceeding twin has more).  Then contains() at the window's
    end: (2, 1) names (1, W), the last bit, and executes; (2, 2) names (1, W + 1), one past, and waits.  Then the
    release: (1, 1) executes at offset 0 into a full window and the frontier jumps to W, where it sticks again;
    (1, 2 W) sits on the new window's last bit, (2, 3) names it and executes, (2, 4) names the seq below and
    waits.  after: (1, W + 1) arrives last, at offset 0 under an exception, and releases (2, 2)."""
    head, rel = stuck_head(held)
    rows = head + [((1, q), []) for q in range(2, W + 1)]
    if extra:
        rows.append(((1, W + 1), []))
    rows += [((2, 1), [(1, W)]), ((2, 2), [(1, W + 1)])]
    if release:
        rows += [rel, ((1, 2 * W), []), ((2, 3), [(1, 2 * W)]), ((2, 4), [(1, 2 * W - 1)])]
    if after:
        rows.append(((1, W + 1), []))
    return T(rows)


def window(tier):
    W = R.tier_limits(tier, N).W
    held = tier != WIDE
    streams = [stuck(W, False, held=held), stuck(W, True, held=held), stuck(W, False, release=False, held=held),
               stuck(W, False, held=held, after=True)]
    return Case("window %s" % R.TIER_NAME[tier], streams, [tier],
                [Pair(0, 1, "window", tier, W if held else W - 1, "off_pop" if tier in (WIDE, WIDE_HBM) else "off",
                      W - 1)])


def words_stream(E, gap, held):
    """E executed exceptions (1, 2) .. above a stuck frontier (gap: but that seq), then the release: the frontier
    runs over them (to the gap) and the rest of the window shifts down across its words.  Then what the window
    holds, read back through deps: the last exception, the seq past it, the gap, the seq after the gap."""
    top = E + 1 + (1 if gap else 0)
    head, rel = stuck_head(held)
    rows = head + [((1, q), []) for q in range(2, top + 1) if q != gap]
    rows.append(rel)
    probes = [top, top + 1] + ([gap, gap + 1, gap - 1] if gap else [])
    rows += [((2, j + 1), [(1, q)]) for j, q in enumerate(probes)]
    if gap:
        rows.append(((1, gap), []))
    rows += [((1, top + 1), []), ((3, 1), [(1, top + 1), (1, top + 2)])]
    return T(rows)


def words(tier):
    """The multi-word windows: 31 / 32 / 33 and 63 / 64 / 65 exceptions, and the last word (W - 33, W - 32, W - 2),
    each whole and with a gap one word in, so that the frontier's walk and the shift end inside a word."""
    W = R.tier_limits(tier, N).W
    held = tier != WIDE
    counts = sorted(set(e for e in (31, 32, 33, 63, 64, 65, W - 33, W - 32, W - 2) if 0 < e < W - 1))
    streams = [words_stream(E, 0, held) for E in counts] + [words_stream(E, 34, held) for E in counts if E > 40]
    return Case("words %s" % R.TIER_NAME[tier], streams, [tier])


# ------------------------------------------------------------------ the largest cascades
def ring(K, waiter):
    """K commands in one cycle, each naming the next, the last closing it: one SCC of K vertices found by a search
    K frames deep, K ids, K dots on the worklist at once (waiter: one vertex fewer in the cycle, and a command
    that names its lowest dot and comes in between)."""
    dots = [spread(i) for i in range(K)]
    rows = [(dots[i], [dots[(i + 1) % K]]) for i in range(K)]
    if waiter:
        rows.insert(K // 2, ((N, 7), [dots[0]]))
    return T(rows + [(spread(K), [dots[0]])])


def worklist(tier):
    lim = R.tier_limits(tier, N)
    K = lim.P
    return Case("worklist %s" % R.TIER_NAME[tier], [ring(K, False), ring(K - 1, True), slots(tier).streams[0]], [tier])


# ------------------------------------------------------------------ placement in a batch
def mixed(seed, L, n=N, maxdeps=3):
    """A seeded stream of L Adds that fits every tier (at most 10 pending; the seed is stepped until it does): deps
    among nearby dots, a few of them never committed, arrivals shuffled a little."""
    while True:
        rng = random.Random(seed)
        dots = [spread(i, n) for i in range(L + 3)]
        order = sorted(range(L + 3), key=lambda i: i + rng.random() * 5)[:L]
        rows = []
        for i in order:
            near = [j for j in range(max(0, i - 4), min(L + 3, i + 3)) if j != i]
            rows.append((dots[i], [dots[j] for j in rng.sample(near, min(len(near), rng.randrange(0, maxdeps + 1)))]))
        if R.run(T(rows), n)["stats"]["slots_all"] <= 10:
            return T(rows)
        seed += 7919


PLACES = (0, 15, 16, 63, 64)
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 17, 23)


def placement(tier, S):
    """A stream the tier stops (slots, P + 1) at streams 0, 15, 16, 63, 64 and the last; fitting streams of
    different lengths, 0 and 1 among them, between."""
    stop = slots(tier).streams[1]
    at = set(s for s in PLACES + (S - 1,) if s < S)
    streams = [stop if s in at else mixed(1000 * S + s, LENGTHS[(s + S) % len(LENGTHS)]) for s in range(S)]
    return Case("placement %s S=%d" % (R.TIER_NAME[tier], S), streams, [tier])


def split_tiles():
    """Three tiles (130 streams): tile 0 of single deps (the lane kernel), tile 1 of three deps an Add (the group
    kernel), the ragged tile 2 light again.  In each, one stream that waits 13 deep -- too many for the lane
    kernel's 12 slots, not for the group kernel's 16 -- and in tile 1 one that waits 17 deep."""
    deep = lambda K, on: T([(spread(i), on) for i in range(K)] + [(d, []) for d in on])
    light, heavy = [(N, 1)], [(N, 1), (N, 2), (N, 3)]
    streams = [mixed(7000 + s, LENGTHS[s % len(LENGTHS)], maxdeps=1) for s in range(64)]
    streams += [deep(4 + s % 9, heavy) for s in range(64)]
    streams += [mixed(7200 + s, LENGTHS[s % len(LENGTHS)], maxdeps=1) for s in range(2)]
    streams[5], streams[63] = deep(13, light), deep(12, light)
    streams[64 + 15], streams[64 + 16], streams[64 + 63] = deep(13, heavy), deep(17, heavy), deep(16, heavy)
    streams[129] = deep(13, light)
    return Case("split tiles", streams, [SPLIT])


# ------------------------------------------------------------------ resume
def resume_cuts(tier):
    """(case, cut rows, (slots row, window row, pending at the window row)): a stream cut where its slot table is
    full (at the slots row, and a row to either side), one cut where a window word is full (31, 32 and 33
    exceptions) and where the whole window is (the window row) and again after the release, and one cut while a
    vertex with exactly C cached deps waits (rows 1 and 2).  FX_TIER_WIDE_HBM at its own sizes: all 16384
    vertices taken (slots_apart) and all 32768 bits walked (window_late); its third stream is the slot tiers'
    largest cascade."""
    lim = R.tier_limits(tier, N)
    b = (N, 1)
    if tier == WIDE_HBM:
        K = R.tier_limits(GLOBAL, N).P
        streams = [slots_apart(tier).streams[0], window_late(tier).streams[0], T(waiting(K, b) + [(b, [])])]
        slots_row, window_row, held = lim.P, lim.W - 1, 0  # the frontier is held back by a late seq: row q - 2
    else:
        K = slots_held(lim)
        full = T(waiting(K, b) + [(b, [])] + [(spread(K + i), []) for i in range(3)])
        streams = [full, stuck(lim.W, False), cache(tier).streams[0] if R.CACHE[tier] else full]
        slots_row, window_row, held = K, lim.W, 1
    case = Case("resume %s" % R.TIER_NAME[tier], streams, [tier])
    cuts = [1, 2, 31, 32, 33, 34, slots_row - 1, slots_row, slots_row + 1, window_row, window_row + 2, window_row + 3]
    return case, sorted(set(c for c in cuts if c > 0)), (slots_row, window_row, held)


def slots_apart(tier):
    """Each command waits on a dot of its own that never arrives: P vertices and no cascade (the docstring); one
    more stops the tier.  The fitting stream ends with every vertex pending."""
    lim = R.tier_limits(tier, N)
    st = lambda K: T([(spread(i), [(N, i + 1)]) for i in range(K)])
    return Case("slots apart %s" % R.TIER_NAME[tier], [st(lim.P), st(lim.P + 1)], [tier],
                [Pair(0, 1, "slots", tier, lim.P, "slots_all", lim.P)])


def window_late(tier):
    """window() with the frontier held back by a late seq: the HBM wide tier's index has as many slots a source
    as its window has bits, so a pending (1, 1) would share its slot with the seq one past the window."""
    W = R.tier_limits(tier, N).W
    streams = [stuck(W, False, held=False), stuck(W, True, held=False), stuck(W, False, held=False, after=True)]
    return Case("window %s" % R.TIER_NAME[tier], streams, [tier], [Pair(0, 1, "window", tier, W - 1, "off_pop", W - 1)])


def tier_cases(tier):
    cases = [slots(tier), slots_reuse(tier), window(tier), worklist(tier), widest(tier)]
    if tier != WIDE:
        cases.append(cache(tier) if tier != LANE_REG else slots(tier, 8))
    if R.tier_limits(tier, N).W > 32:
        cases.append(words(tier))
    return cases


@functools.lru_cache(None)
def all_cases():
    """The cases that fit some tier of the ladder: single launches, and fx_batch_run_tiered from any tier."""
    cases = [c for tier in LIMITED for c in tier_cases(tier)]
    cases += [placement(tier, S) for tier in LIMITED for S in (1, 63, 65, 130)]
    cases.append(split_tiles())
    return cases


@functools.lru_cache(None)
def hbm_cases():
    """FX_TIER_WIDE_HBM at its own sizes: the last tier, so its exceeding streams fit nowhere (single launches)."""
    return [slots_apart(WIDE_HBM), window_late(WIDE_HBM)]
