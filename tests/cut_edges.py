"""The cut driver's edge cases (test infrastructure): hand-built batches, each
the smallest that sits on one limit of the cut analysis of
fantoch_amd/csrc/graph_cut.hip (fx_batch_run_cut), named after that limit.
Shared by the CPU tests (test_cut_edges_ref.py: the restatement cut_ref
against the oracle, that every case reaches its limit and tells a wrong
restatement from the right one) and the GPU tests (test_cut_edges_gpu.py).

A stream is laid out with numpy straight into a `Planes` (St, pack): the Add
at step p has the dot (1 + p % n, 1 + p // n) unless a case names another, and
t_ms = p.  A segment of up to 130 Adds is a cycle (Add j names Add j + 1, the
last the first); a longer one is a chain: its first Add names the dot of its
last and the others have no dep, so the executor holds one vertex while the
segment lasts.

What a case expects of a launch over buffers of 0xA5 (Case.want): every
stream's executed rows of order, the release rows of its Adds, nexec and err
are the oracle's on the unsplit stream, and every other word keeps 0xA5.  Two
kinds of stream end in an error every tier reports where the oracle has none
or stops likewise: a dot of a source outside 1..n (FX_ERR_DOT_RANGE, which the
oracle does not check) and a double dot (FX_ERR_DOUBLE_INDEX).  For those the
oracle runs the rows before the stopping row, the rows after it keep 0xA5, and
the stopping row's own release word is left open (graph_edges.check_stopped).
"""
import functools

import numpy as np

import cut_ref as R
from fantoch_amd import _lib
from fantoch_amd import streams as fs
from oracle import oracle_lib

FILL = 0xA5
A5 = 0xA5A5A5A5
NAMES = ("order", "release", "nexec", "err")
CYCLE_MAX = 130  # longer segments are chains


def pk(src, seq):
    return _lib.pack_dot(src, seq)


class St:
    """One stream under construction: positional dots, deps as (row, packed dot) pairs."""

    def __init__(self, n):
        self.n, self.L = n, 0
        self.rows, self.vals = [], []
        self.dots, self.kinds = {}, {}
        self.laid = []  # the segments' lengths as laid down (None once a dep is put by hand)

    def dot(self, p):
        """The packed dot of step p (a number or an array)."""
        p = np.asarray(p, np.int64)
        d = ((1 + p % self.n) << _lib.FX_SEQ_BITS) | (1 + p // self.n)
        if d.ndim == 0:
            return self.dots.get(int(p), int(d))
        d = d.copy()
        for q, v in self.dots.items():
            d[p == q] = v
        return d

    def dep(self, rows, dots):
        self.rows.append(np.atleast_1d(np.asarray(rows, np.int64)))
        self.vals.append(np.atleast_1d(np.asarray(dots, np.int64)))
        return self

    def reach(self, i, j):
        """Step i names the dot of step j."""
        self.laid = None
        return self.dep(i, self.dot(j))

    def singles(self, k):
        self.L += k
        if self.laid is not None:
            self.laid += [1] * k
        return self

    def cycle(self, k):
        a = self.L
        self.L += k
        if self.laid is not None:
            self.laid.append(k)
        j = np.arange(k)
        return self.dep(a + j, self.dot(a + (j + 1) % k))

    def chain(self, k):
        a, laid = self.L, self.laid
        self.L += k
        self.reach(a, a + k - 1)
        self.laid = laid + [k] if laid is not None else None
        return self

    def segs(self, lengths):
        for k in lengths:
            k = int(k)
            self.singles(1) if k == 1 else self.cycle(k) if k <= CYCLE_MAX else self.chain(k)
        return self

    def add(self, dot, deps=()):
        """One Add with a dot of its own and deps given as (source, seq)."""
        self.dots[self.L], self.laid = pk(*dot), None
        self.dep([self.L] * len(deps), [pk(*d) for d in deps])
        self.L += 1
        return self

    def set_dot(self, p, dot):
        self.dots[p] = pk(*dot)
        return self

    def set_kind(self, p, kind):
        self.kinds[p] = kind
        return self

    def arrays(self):
        """(dot [L], rows, vals): the deps of a row ascending and without duplicates (canonical C1)."""
        dot = self.dot(np.arange(self.L)).astype(np.uint32)
        if not self.rows:
            return dot, np.zeros(0, np.int64), np.zeros(0, np.int64)
        key = np.unique((np.concatenate(self.rows) << 32) | np.concatenate(self.vals))
        assert (key >> 32).max() < self.L, "a dep on a row past the stream's end"
        return dot, key >> 32, key & 0xFFFFFFFF


def pack(streams, n, dmax=None, steps=None):
    """The streams as a Planes (lengths always given), filled without a loop over the Adds."""
    built = [st.arrays() for st in streams]
    steps = steps or max([st.L for st in streams] + [1])
    widest = max([int(np.bincount(rows).max()) for _, rows, _ in built if len(rows)] + [0])
    if dmax is None:
        dmax = max(widest, 1)
    assert widest <= dmax
    p = fs.Planes(len(streams), steps, dmax, n, lengths=np.array([st.L for st in streams], np.uint32))
    for s, (st, (dot, rows, vals)) in enumerate(zip(streams, built)):
        if not st.L:
            continue
        at = _lib.index(np.arange(st.L), s, steps)
        p.dot[at] = dot
        nd = np.bincount(rows, minlength=st.L).astype(np.uint32)
        kind = np.zeros(st.L, np.uint32)
        for q, k in st.kinds.items():
            kind[q] = k
        p.hdr[at] = np.arange(st.L, dtype=np.uint32) | (nd << 24) | (kind << 29)  # ascending t_ms below 2^24
        if len(rows):
            j = np.arange(len(rows)) - np.searchsorted(rows, rows, "left")
            p.deps[j * p.plane + at[rows]] = vals
    p.laid = [st.laid for st in streams]
    return p


class Case:
    def __init__(self, name, limit, build, at_commit=False, hists=False, beyond_tiered=()):
        """beyond_tiered: the streams fx_batch_run_tiered itself cannot run (seqs so sparse that an executed dot
        lies above every tier's window: FX_ERR_CAPACITY after the last tier), which the cut driver can, since
        it renumbers a segment's dots densely."""
        self.name, self.limit, self._build, self.at_commit, self.hists = name, limit, build, at_commit, hists
        self.beyond_tiered = tuple(beyond_tiered)
        self._planes = self._analysis = self._oracle = self._stops = None

    def planes(self):
        if self._planes is None:
            self._planes = self._build()
        return self._planes

    def analysis(self):
        if self._analysis is None:
            self._analysis = R.analyse(self.planes())
        return self._analysis

    def stops(self):
        """{stream: (row, err)}: the streams every tier stops with an error at a row (the module docstring)."""
        if self._stops is None:
            self._stops = {}
            for st in self.analysis().streams:
                src = st.dot >> _lib.FX_SEQ_BITS
                rows = [(int(r), _lib.FX_ERR_DOT_RANGE) for r in np.flatnonzero((src < 1) | (src > st.n))[:1]]
                seen = np.flatnonzero(st.table[1:] == st.table[:-1])  # the stable sort keeps equal dots in step order
                if len(seen):
                    rows.append((int(st.table_pos[seen + 1].min()), _lib.FX_ERR_DOUBLE_INDEX))
                if rows and not self.at_commit:
                    self._stops[st.s] = min(rows)
        return self._stops

    def oracle(self):
        """(order, release, nexec, err) of the C++ oracle, a stopped stream cut before its stopping row."""
        if self._oracle is None:
            p = self.planes()
            lengths = p.lengths.copy()
            for s, (row, _) in self.stops().items():
                lengths[s] = row
            q = fs.Planes(p.S, p.steps, p.dmax, p.n, p.dot, p.hdr, p.deps, lengths)
            self._oracle = oracle_lib.batch_execute(q, execute_at_commit=self.at_commit, threads=8)
            for a in self._oracle:
                a.setflags(write=False)
        return self._oracle

    def want(self):
        """(want, open): the four outputs a launch must leave over 0xA5, and the release words left open."""
        p = self.planes()
        order, release, nexec, err = self.oracle()
        want = dict(order=np.full(p.plane, A5, np.uint32), release=np.full(p.plane, A5, np.uint32),
                    nexec=nexec.copy(), err=err.copy())
        left = []
        for s in range(p.S):
            L = int(p.lengths[s])
            if s in self.stops():
                L, want["err"][s] = self.stops()[s]
                left.append(int(_lib.index(L, s, p.steps)))
            rows = _lib.index(np.arange(int(nexec[s])), s, p.steps)
            want["order"][rows] = order[rows]
            rows = _lib.index(np.arange(L), s, p.steps)
            want["release"][rows] = release[rows]
        return want, np.array(left, np.int64)

    def status(self):
        """The call's status: that of the lowest stream with one (run_ladder's k_first_error)."""
        err = self.want()[0]["err"]
        bad = np.flatnonzero(err)
        return int(err[bad[0]]) if len(bad) else _lib.FX_OK

    def first_tier(self):
        """Where fx_batch_run_tiered starts the segment batch (graph_tiers.hip run_tiered): FX_TIER_DEFAULT, or
        FX_TIER_LDS_LARGE for Adds wider than the split tier reads (16)."""
        return _lib.FX_TIER_SPLIT if self.planes().dmax <= 16 else 1

    def reruns_possible(self):
        """A segment of more than 8 Adds may pass a tier's tables (12 slots, a 32-bit window at the lane tier)
        and be rerun one tier up, where tier_counts counts it again."""
        a = self.analysis()
        return any(a.class_counts[4:]) or self.planes().dmax > 8


def through_segments(case, by_source=True):
    """The driver's plan carried out by the oracle: {stream: (order [L], release [L])} for every cut stream, its
    one-Add segments written as k_build writes them, the longer ones renumbered (cut_ref.renumber), run by the
    oracle from an empty graph as one batch and mapped back by their first step as k_scatter does."""
    p, a = case.planes(), case.analysis()
    cut = [st for st in a.streams if not st.whole]
    got = {st.s: (np.arange(st.L, dtype=np.uint32) | np.uint32(_lib.FX_ORDER_SCC_START), np.arange(st.L, dtype=np.uint32))
           for st in cut}
    segs = [(st, int(k)) for st in cut for k in np.flatnonzero(st.length > 1)]
    if not segs:
        return got
    batch = fs.pack_streams([st.renumber(k, by_source) for st, k in segs], p.n)
    order, release, nexec, err = oracle_lib.batch_execute(batch, threads=8)
    for b, (st, k) in enumerate(segs):
        a0, n = int(st.start[k]), int(st.length[k])
        assert (int(nexec[b]), int(err[b])) == (n, 0), "%s: segment %d of stream %d does not execute completely" % (
            case.name, k, st.s)
        rows = _lib.index(np.arange(n), b, batch.steps)
        o = order[rows]
        got[st.s][0][a0:a0 + n] = (a0 + (o & np.uint32(0x7FFFFFFF))) | (o & np.uint32(_lib.FX_ORDER_SCC_START))
        got[st.s][1][a0:a0 + n] = a0 + release[rows]
    return got


# ------------------------------------------------------------------ the cases
def mixed(n, L, seed):
    """A stream of exactly L Adds: singles and cycles of 2, 3 and 5, seeded."""
    rng = np.random.default_rng(seed)
    st = St(n)
    while st.L < L:
        k = int(rng.choice([1, 1, 1, 2, 3, 5]))
        st.segs([k if st.L + k <= L else 1])
    return st


def block_edge():
    n, steps = 5, 2 * R.CHUNK + 3
    e = R.CHUNK
    sts = [St(n).singles(L - 2).cycle(2) for L in (e - 1, e, e + 1)]  # the last flag on either side of the edge
    sts.append(St(n).singles(e - 2).cycle(4).singles(steps - e - 2))  # a 4-cycle on e - 2 .. e + 1
    sts.append(St(n).singles(e - 2).cycle(2).cycle(2).singles(steps - e - 2))  # a cut at e - 1, a 2-cycle after it
    sts.append(St(n).singles(steps).reach(5, e + 6))  # the carry goes into block 1
    sts.append(St(n).singles(steps).reach(e - 24, steps - 1))  # .. and through block 1, which adds nothing
    return pack(sts, n)


def max_seg():
    n, M = 5, R.MAX_SEG
    exact = St(n).segs([1, 1, 2, M, 1, 3, 1])
    over = St(n).segs([1, 1, 2, 1, 3, 1, 1, 5, M + 1, 1, 2])  # singles and short segments before its long one
    bounds = []
    for c in range(1, 12):
        bounds += [1 << c, (1 << c) + 1, 1]
    every = St(n).segs(bounds[:-1])  # 2, 3, 4, 5, 8, 9, .. 2048, 2049
    return pack([exact, over, every], n)


def streams(S, steps):
    n = 5
    lengths = [(7 * s + 3) % (steps + 1) for s in range(S)]  # ragged, with 0, 1 and steps among them
    for s, L in ((S // 3, 1), (S // 2, 0), (S - 1, steps)):
        lengths[s] = L
    return pack([mixed(n, L, 100 * S + s) for s, L in enumerate(lengths)], n, steps=steps)


def chunks64(steps):
    n, e = 5, R.CHUNK
    across = St(n).singles(steps)
    for k in range(1, (steps - 1) // e + 1):  # a 2-cycle across every multiple of 1,024
        across.reach(k * e - 1, k * e).reach(k * e, k * e - 1)
    into = St(n).singles(steps - 1)  # reaches into the next block and the one after
    for i, j in ((1000, 1030), (3000, 5000), (10230, 10250), (30000, 32769), (64000, steps - 2)):
        into.reach(i, j)
    return pack([across, into], n)


def rounds():
    """steps = 2^20 + 1025 (nch = 1026): k_chunk_excl_blk's second round holds two chunks."""
    n, r = 5, R.CHUNK * R.CHUNK
    st = St(n).singles(r + R.CHUNK + 1)
    for j in range(4):  # a 4-cycle on r - 2 .. r + 1
        st.reach(r - 2 + j, r - 2 + (j + 1) % 4)
    st.reach(r - 6, r + 4)
    # a 2-cycle at either end: the later one's segment id lies past 2^20, so its batch slot needs the carry of
    # the sum scans (k_segs' ccnt_excl, the class scan) between rounds as well
    st.reach(10, 11).reach(11, 10).reach(st.L - 2, st.L - 1).reach(st.L - 1, st.L - 2)
    return pack([st], n)


CLASS_RUN = (2, 3, 5, 9, 17, 33, 65)  # classes 1 .. 7


def class_chunks(NS):
    n = 5
    lens = [1] * NS
    for i, k in ((63, 2), (64, 3), (255, 4), (256, 5), (1023, 2), (1024, 9), (2047, 3), (2048, 2)):
        if i < NS:
            lens[i] = k
    for i in range(64):  # one wave of k_class_fill: 64 consecutive segments, classes cycling 1 .. 7
        lens[320 + i] = CLASS_RUN[i % 7]
    return pack([St(n).segs(lens[:70]), St(n).segs(lens[70:])], n)


RANKED = (4, 5, 8, 9, 17)


def rank_path(steps):
    n = 5
    lens = [1] * 7
    for k in RANKED:
        lens += [k, 1, 1]
    lens += [1] * (steps - sum(lens))
    return pack([St(n).segs(lens)], n)


SPARSE = [((2, 5), (3, 7), (2, 900000), (3, 1), (2, 17)), ((5, 50), (5, 1000000), (5, 60))]


def dots8():
    n = 8
    sparse = St(n).add((1, 1)).add((4, 1))
    for ring in SPARSE:  # seqs sparse inside one segment: a cycle ranked by k_rank, one ranked by k_build
        for j, d in enumerate(ring):
            sparse.add(d, [ring[(j + 1) % len(ring)]])
        sparse.add((1, 2 + SPARSE.index(ring)))
    wide = St(n)
    before = [(1 + j % 5, 1 + j // 5) for j in range(25)]
    after = [(7, j + 1) for j in range(6)]
    for d in before:
        wide.add(d)
    wide.add((6, 1), before + after)  # 31 deps: 25 in the executed prefix, 6 in its segment
    for d in after:
        wide.add(d)
    wide.add((8, 1), [(6, 1)])
    own = St(n).add((1, 1), [(1, 1)]).add((2, 1)).add((3, 1), [(3, 1), (4, 1)]).add((4, 1), [(3, 1)]).add((2, 2))

    def never(dep):
        """(1, 7) is the stream's highest seq; source 2 ends at (2, 3)."""
        st = St(n).add((1, 1)).add((2, 1)).add((2, 2), [(2, 3)]).add((2, 3), [(2, 2)])
        for q in range(2, 8):
            st.add((1, q))
        return st.add((3, 1), [dep]).add((3, 2)).add((4, 1), [(4, 2)]).add((4, 2), [(4, 1)])

    plain = St(n).add((1, 1)).add((2, 1), [(3, 1)]).add((3, 1), [(2, 1)]).add((1, 2))
    return pack([sparse, never((0, 1)), wide, never((n + 1, 1)), own, never((1, 8)), plain, never((2, 7)), plain], n)


def dots1():
    return pack([St(1).segs([1, 2, 1, 1, 5, 9, 1]), St(1).segs([3, 1, 17, 1])], 1)


def dmax0():
    p = pack([St(3).singles(9), St(3).singles(6), St(3).singles(0)], 3)
    q = fs.Planes(p.S, p.steps, 0, p.n, p.dot, p.hdr, None, p.lengths)  # built directly: pack_streams has dmax >= 1
    q.laid = p.laid
    return q


BEFORE = [1, 1, 2, 1, 3, 1]  # what every spoiled stream has before the step that spoils it
AFTER = [1, 2, 1]


def whole_beside_cut():
    n = 5
    at = sum(BEFORE)
    spoiled = [
        St(n).segs(BEFORE + [1] + AFTER).set_dot(at, (n + 1, 1)),  # a dot source outside 1..n
        St(n).segs(BEFORE + [3] + AFTER).set_dot(at + 2, (1 + at % n, 1 + at // n)),  # a double dot, of a pending one
        St(n).segs(BEFORE + [1] + AFTER).set_kind(at, _lib.FX_KIND_INDEX_ONLY),  # a record that is not an Add
        St(n).segs(BEFORE + [1] + AFTER).dep(at, pk(2, 9999)),  # a dep that never arrives: no cut at the last step
        St(n).segs(BEFORE + [R.MAX_SEG + 1] + AFTER),  # a segment over MAX_SEG
    ]
    sts = [mixed(n, 40, 900)]
    for i, st in enumerate(spoiled):
        sts += [st, mixed(n, 37 + i, 901 + i)]
    return pack(sts, n)


def sparse_fallback():
    """33 streams whose highest seq is 0xFFFFFF: a position table of 33 * 8 * 2^24 > 2^32 words.  The Add with
    that seq waits on a dot that never arrives: executed, it would lie 2^24 above its source's frontier, past
    every tier's window."""
    n = 8
    return pack([St(n).add((1, 1)).add((2, _lib.FX_SEQ_MASK), [(1, 2)]) for _ in range(33)], n)


def at_commit():
    return pack([mixed(3, L, 50 + L) for L in (9, 0, 14)], 3)


@functools.lru_cache(None)
def all_cases():
    cases = [Case("block edge", "CHUNK", block_edge, hists=True), Case("MAX_SEG", "MAX_SEG", max_seg, hists=True)]
    cases += [Case("streams S=%d" % S, "SMALL_S / FX_TILE_STREAMS", functools.partial(streams, S, steps))
              for S, steps in ((1, 41), (63, 42), (64, 43), (65, 44), (130, 45))]
    cases += [Case("64 chunks steps=%d" % steps, "nch > 64", functools.partial(chunks64, steps))
              for steps in (R.BLK_ABOVE * R.CHUNK, R.BLK_ABOVE * R.CHUNK + 1)]
    cases += [Case("class chunks NS=%d" % NS, "class chunks", functools.partial(class_chunks, NS))
              for NS in (1023, 1024, 1025, 2049)]
    cases += [Case("rank path steps=%d" % steps, "nl_adds * 8 < work", functools.partial(rank_path, steps))
              for steps in (512, 513)]
    cases += [Case("dots n=8", "dots", dots8, beyond_tiered=(0,)), Case("dots n=1", "dots", dots1), Case("dots dmax=0", "dots", dmax0),
              Case("whole beside cut", "whole", whole_beside_cut),
              Case("sparse fallback", "ptotal > 2^32", sparse_fallback),
              Case("execute at commit", "execute at commit", at_commit, at_commit=True)]
    return cases


def rounds_case():
    """Five planes of 268 MB: built where it is used and dropped after, not kept with all_cases()."""
    return Case("rounds", "nch > 1024", rounds)
