"""CPU restatement of Caesar's PredecessorsGraph, with the limits of the
device tables (test infrastructure).  Written from the reference's
fantoch_ps/src/executor/pred/mod.rs:104-383 and index.rs:96-120 (cited lines
are mod.rs unless another file is named), not from oracle/pred_oracle.cpp.
What fx_pred_execute / fx_pred_run are compared against, bit for bit.

A stream is a list of Adds (dot, deps, t_ms, clock): dot = (source, seq),
deps a collection of dots, clock = (seq, process id), compared as the pair
(common/pred/clocks/mod.rs:15-30).

Precondition: the deps of an Add are distinct (canonical C1; the packers sort
and deduplicate them) and do not hold the Add's own dot (:126).

Canonicalisation: the waiters a PendingIndex::remove returns (a HashSet,
index.rs:117-119) are visited ascending by dot (C2).

run(stream, n, limits=None): the unbounded semantics.  With limits (a Limits,
see `tier_limits`): the same, stopped with FX_ERR_CAPACITY where a table of that
size ends, counted as fantoch_amd/csrc/pred_exec.hip counts:
  vertices  a commit with P commands pending (the index and the window of
            that commit are checked before it)
  index     a commit whose seq mod Q is that of a pending dot of its source
  window    a commit (committed clock) or an execution (executed clock) with
            seq - frontier - 1 >= W.  Neither is recorded: a commit beyond
            the committed window executes nothing (also under
            execute_at_commit), an execution beyond the executed window
            leaves order, release and nexec as they were
  frames    a PendingIndex::remove at recursion depth FD (live frames: one per
            enclosing try_phase_*_pending loop over a non-empty set, an
            exhausted one included until the recursion unwinds), made while
            that phase's index holds any registration: the depth is tested
            before the removal, so one that would find no waiter stops too
  lists     the waiter sets of all live frames together exceed LL entries
What the reference leaves to a panic, defined here:
  FX_ERR_DOT_RANGE     a committed dot with source 0, source above n, or seq 0
  FX_ERR_DOUBLE_INDEX  a second commit of a dot (:123), also after it executed
The first failing row ends the stream; what executed before it stands.
"non-executed dependency must exist" (:242) cannot fail: a committed dot is
indexed before anything else of its Add (:132) and leaves the index only in
save_to_execute (:350-353), which marks it executed (:363); here it is an
AssertionError.
"""
import collections
import sys

FX_OK, FX_ERR_CAPACITY, FX_ERR_DOUBLE_INDEX, FX_ERR_DOT_RANGE = 0, 2, 3, 5
FX_RELEASE_NONE = 0xFFFFFFFF
SCC_START = 0x80000000
SMALL, LDS, HBM = 0, 1, 2  # FX_PRED_TIER_*
TIER_NAME = {SMALL: "SMALL", LDS: "LDS", HBM: "HBM"}
RESOURCES = ("vertices", "index", "window", "frames", "lists")

Limits = collections.namedtuple("Limits", "P Q W FD LL")


def lay_words(P, Q, WB, n, D, LL, FD=0):
    """Lay::make (pred_exec.hip): the words of one stream's tables."""
    DW, FD = (D + 31) // 32, FD or P
    return 6 * P + 2 * P * DW + P * D + P + n * Q + 8 + n * WB + 8 + n * WB + FD * 4 + LL + P


def tier_limits(tier, n, dmax):
    """pred_layout / small_fixed_layout (pred_exec.hip) as Limits; None when the tier's tables do not fit."""
    D, lds = max(dmax, 1), 160 * 1024 // 4
    if tier == HBM:
        return Limits(8192, 16384, 1024 * 32, 8192, 8 * 8192)
    if tier == SMALL:
        if n == 5 and D == 5:  # the compiled layout: FX_PRED_Q, FX_PRED_WB, FX_PRED_FRAMES, FX_PRED_LISTS
            return Limits(64, 32, 8 * 32, 32, 96)
        return Limits(64, 128, 32 * 32, 64, 4 * 64) if lay_words(64, 128, 32, n, D, 256) <= lds else None
    for P in (512, 256, 128):
        if lay_words(P, 2 * P, 64, n, D, 4 * P) <= lds:
            return Limits(P, 2 * P, 64 * 32, P, 4 * P)
    return None


def chain(n, dmax):
    """The tiers fx_pred_run goes through: the ones whose tables fit."""
    return [t for t in (SMALL, LDS, HBM) if tier_limits(t, n, dmax) is not None]


class Stop(Exception):
    def __init__(self, err, resource=None, clock=None):
        self.err, self.resource, self.clock = err, resource, clock


class AEClock:
    """threshold::AEClock of one executor: per source a frontier and the events above it."""

    def __init__(self, n, name, graph):
        self.front, self.above = {p: 0 for p in range(1, n + 1)}, {p: set() for p in range(1, n + 1)}
        self.name, self.g = name, graph

    def contains(self, dot):
        src, seq = dot
        return src in self.front and (seq <= self.front[src] or seq in self.above[src])

    def add(self, dot):
        src, seq = dot
        if self.contains(dot):
            return False
        g = self.g
        g.peak["window"] = max(g.peak["window"], seq - self.front[src])
        if g.lim and seq - self.front[src] - 1 >= g.lim.W:
            raise Stop(FX_ERR_CAPACITY, "window", self.name)
        self.above[src].add(seq)
        while self.front[src] + 1 in self.above[src]:
            self.front[src] += 1
            self.above[src].discard(self.front[src])
        return True


class Vertex:  # index.rs:10-62
    def __init__(self, dot, rec, clock, deps):
        self.dot, self.rec, self.clock, self.deps, self.missing_deps = dot, rec, clock, deps, 0


class Graph:
    def __init__(self, n, lim=None, at_commit=False):
        self.n, self.lim, self.execute_at_commit = n, lim, at_commit
        self.peak = dict.fromkeys(RESOURCES, 0)
        self.committed_clock, self.executed_clock = AEClock(n, "committed", self), AEClock(n, "executed", self)
        self.vertex_index = {}
        self.pending_seqs, self.slots = {p: set() for p in range(1, n + 1)}, set()  # of vertex_index: the dot index
        self.pending_index = [{}, {}]  # phase one, phase two: dep -> the dots waiting on it
        self.nreg = [0, 0]             # registrations each index holds
        self.depth = self.live = 0     # live frames and their waiters
        self.order, self.release, self.step = [], {}, 0

    def add(self, dot, rec, clock, deps):  # :104-152
        src, seq = dot
        if src < 1 or src > self.n or seq == 0:
            raise Stop(FX_ERR_DOT_RANGE)
        if self.committed_clock.contains(dot):  # :123
            raise Stop(FX_ERR_DOUBLE_INDEX)
        self.committed_clock.add(dot)
        assert dot not in deps  # :126
        if self.execute_at_commit:
            self.execute(dot, rec)  # :129
            return
        self.index_committed_command(dot, rec, clock, deps)
        self.try_pending(0, dot)  # :136
        self.move_to_phase_one(dot)  # :139

    def index_committed_command(self, dot, rec, clock, deps):  # :277-293
        assert dot not in self.vertex_index
        lim = self.lim
        same = self.pending_seqs[dot[0]]  # the pending seqs of this source
        span = max(max(same, default=dot[1]), dot[1]) - min(min(same, default=dot[1]), dot[1]) + 1
        self.peak["index"] = max(self.peak["index"], span)  # <= Q: no two of them share seq mod Q
        if lim and (dot[0], dot[1] % lim.Q) in self.slots:
            raise Stop(FX_ERR_CAPACITY, "index")
        self.peak["vertices"] = max(self.peak["vertices"], len(self.vertex_index) + 1)
        if lim and len(self.vertex_index) >= lim.P:
            raise Stop(FX_ERR_CAPACITY, "vertices")
        self.vertex_index[dot] = Vertex(dot, rec, clock, deps)
        same.add(dot[1])
        if lim:
            self.slots.add((dot[0], dot[1] % lim.Q))

    def move_to_phase_one(self, dot):  # :154-206
        vertex = self.vertex_index[dot]
        non_committed = [d for d in vertex.deps if not self.committed_clock.contains(d)]
        for d in non_committed:
            self.pending_index[0].setdefault(d, set()).add(dot)  # index.rs:112-114
        self.nreg[0] += len(non_committed)
        if non_committed:
            vertex.missing_deps = len(non_committed)
        else:
            self.move_to_phase_two(dot)

    def move_to_phase_two(self, dot):  # :208-275
        vertex = self.vertex_index[dot]
        count = 0
        for d in vertex.deps:
            if not self.executed_clock.contains(d):
                assert d in self.vertex_index, "non-executed dependency must exist"  # :242
                if self.vertex_index[d].clock < vertex.clock:  # :246
                    count += 1
                    self.pending_index[1].setdefault(d, set()).add(dot)
        self.nreg[1] += count
        if count:
            vertex.missing_deps = count
        else:
            self.save_to_execute(dot)

    def try_pending(self, ph, dot):
        """try_phase_one_pending (:295-316, ph 0) / try_phase_two_pending (:318-339, ph 1)."""
        lim = self.lim
        if self.nreg[ph] == 0:
            return  # an empty index: no frame is needed
        self.peak["frames"] = max(self.peak["frames"], self.depth + 1)
        if lim and self.depth >= lim.FD:
            raise Stop(FX_ERR_CAPACITY, "frames")
        waiters = self.pending_index[ph].pop(dot, set())  # index.rs:117-119
        self.nreg[ph] -= len(waiters)
        if not waiters:
            return
        self.peak["lists"] = max(self.peak["lists"], self.live + len(waiters))
        if lim and self.live + len(waiters) > lim.LL:
            raise Stop(FX_ERR_CAPACITY, "lists")
        self.depth, self.live = self.depth + 1, self.live + len(waiters)
        for pending_dot in sorted(waiters):
            vertex = self.vertex_index[pending_dot]
            assert vertex.missing_deps > 0  # index.rs:52
            vertex.missing_deps -= 1
            if vertex.missing_deps == 0:
                if ph == 0:
                    self.move_to_phase_two(pending_dot)
                else:
                    self.save_to_execute(pending_dot)
        self.depth, self.live = self.depth - 1, self.live - len(waiters)

    def save_to_execute(self, dot):  # :341-367
        vertex = self.vertex_index.pop(dot)
        self.pending_seqs[dot[0]].discard(dot[1])
        if self.lim:
            self.slots.discard((dot[0], dot[1] % self.lim.Q))
        self.execute(dot, vertex.rec)
        self.try_pending(1, dot)  # :366

    def execute(self, dot, rec):  # :369-383
        assert self.executed_clock.add(dot)  # :379
        self.order.append(rec)
        self.release[rec] = self.step


def run(stream, n, limits=None, at_commit=False):
    """One stream through the graph.  Returns a dict: order (arrival indexes in
    execution order), release (arrival -> executing step; absent: never
    executed, FX_RELEASE_NONE), nexec, err, stop (the resource that stopped
    it, of RESOURCES, else None), clock (which clock's window), row (the row
    that failed, else None), peak (the
    most each resource held or was asked for, the stopping request included:
    vertices pending, index the span of one source's pending seqs, window
    seq - frontier, frames, lists)."""
    g = Graph(n, limits, at_commit)
    err = stop = clock = None
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 40000))
    try:
        for rec, add in enumerate(stream):
            dot, deps, clk = tuple(add[0]), set(tuple(d) for d in add[1]), tuple(add[3])
            g.step = rec
            g.add(dot, rec, clk, deps)
    except Stop as e:
        err, stop, clock = e.err, e.resource, e.clock
    finally:
        sys.setrecursionlimit(old)
    return dict(order=g.order, release=g.release, nexec=len(g.order), err=err or FX_OK, stop=stop, clock=clock,
                row=g.step if err else None, peak=g.peak, pending=len(g.vertex_index))


def run_chain(stream, n, dmax, at_commit=False):
    """fx_pred_run: the stream at each tier that fits while it stops with
    FX_ERR_CAPACITY.  Returns (the last tier's result, reruns)."""
    reruns = -1
    for tier in chain(n, dmax):
        r = run(stream, n, tier_limits(tier, n, dmax), at_commit)
        reruns += 1
        if r["err"] != FX_ERR_CAPACITY:
            break
    return r, reruns
