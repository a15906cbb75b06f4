"""A plain restatement of the graph executor (test infrastructure): the
reference's DependencyGraph as oracle/graph_oracle.cpp restates it -- handle_add,
the vertex index, Tarjan with every SCC saved in ascending dot order,
check_pending / try_pending, the executed AEClock -- that counts, while it
runs a stream, the quantities the tiers of fantoch_amd/csrc/graph_*.hip
compare with a table size, each at the moment and in the way the kernels
test it, and that stops a stream at the row where a tier would stop it.

A stream is a list of Adds (dot, deps, t_ms[, kind]) with dot = (source, seq).

The counters (run(...)["stats"]) and the lines they mirror:
  slots      pending vertices once a new vertex is in, counted where a vertex
             takes a slot: `!fre` in insert_vertex (graph_group.hip:151,
             graph_wave.hip:158, graph_lane.hip:290) and pt_insert
             (graph_exec.hip:236).  An Add whose deps are all executed takes
             the fast path there and no slot.
  slots_all  the same counted for every Add: the wide tiers have no fast
             path, every Add takes a vertex (`!nfree`, graph_wide.hip:684).
  cache      deps kept for a new vertex, those that are not the vertex itself
             and not in the executed clock at that moment: `nc > C`
             (graph_group.hip:157, graph_wave.hip:162), `nc >= T::C` before the
             store in pt_cache_dep (graph_exec.hip:258).
  off        for every clk_add of a seq above its source's frontier, seq -
             frontier - 1, the SCC's members added in ascending dot order:
             `off >= 32u` (graph_group.hip:114, graph_wave.hip:121,
             graph_lane.hip:174), `off >= 32u * T::XW` (graph_exec.hip:179).
  off_pop    the same with an SCC's members added as the wide tiers add them,
             in Tarjan-stack pop order and before the SCC is saved: `sq - f - 1
             >= L.WB * 32u` (graph_wide.hip:224, called from :490).
  wl         high-water mark of check_pending's worklist counted as GROUP,
             WAVE, the slot tiers and the wide tiers count it: a whole SCC is
             added at once (`nwl + cnt > WLC`, graph_group.hip:207,
             graph_wave.hip:210; `nwl + cnt > L.wlcap`, graph_wide.hip:289; the
             slot tiers push unchecked into P + 1 words, graph_exec.hip:68,339),
             the fast path's own dot is entry 0 when anything waits.
  wl_mask    the same counted as LANE_REG counts it: one entry per executed
             dot that has waiters when it executes (wl_push, graph_lane.hip:222,
             called at :519); the fast path's dot is never pushed.
  index      whether an Add's dot shared (source, seq mod 256) with a pending
             dot: the LDS wide tier's index (graph_wide.hip:676-682).  The HBM
             wide tier's index has 32768 slots per source and is not counted:
             no stream of graph_edges has two pending dots of one source
             32768 seqs apart (its window case holds the frontier back with a
             late seq for that reason, graph_edges.window_late).
  max_pending, max_window   what the oracle's stats=True gives: pending
             vertices, and highest executed exception less the frontier, at
             the end of a step.

What is not restated: the wide tiers' waiters per vertex (PW) and missing-dep
list (nml).  Both exist only under FX_FLAG_PARTIAL (graph_wide.hip:447-455,
543-577), which fx_batch_execute refuses (graph_tiers.hip:124) and which has
shard_count > 1; this restatement, like the oracle's batch form, is the
shard_count == 1 graph, where a vertex waits on one dot at a time.
"""
import collections
import ctypes

from fantoch_amd import _lib

FX_ERR_CAPACITY = _lib.FX_ERR_CAPACITY
FX_ERR_DOUBLE_INDEX = _lib.FX_ERR_DOUBLE_INDEX
FX_ERR_DOT_RANGE = _lib.FX_ERR_DOT_RANGE
FX_RELEASE_NONE = _lib.FX_RELEASE_NONE
SCC_START = _lib.FX_ORDER_SCC_START

GROUP, LDS_LARGE, GLOBAL, LANE, WAVE, LANE_REG, SPLIT, WIDE, WIDE_HBM = range(9)  # FX_TIER_* (include/fantoch_amd.h)
TIER_NAME = {GROUP: "GROUP", LDS_LARGE: "LDS_LARGE", GLOBAL: "GLOBAL", LANE: "LANE", WAVE: "WAVE",
             LANE_REG: "LANE_REG", SPLIT: "SPLIT", WIDE: "WIDE", WIDE_HBM: "WIDE_HBM"}

# Cached not-yet-executed deps per vertex; not exported to Python.  GROUP_CACHE (fx_internal.h:95), Tier1's and
# Tier2's C (graph_exec.hip:79-80), TierLane's C (graph_exec.hip:78), WAVE_CACHE (fx_internal.h:105).  LANE_REG
# caches as many deps as it reads (LANE_MAX_DEPS, fx_internal.h:116): no Add it is given outgrows that.  The wide
# tiers keep every dep of the widest Add (graph_wide.hip:75).
CACHE = {GROUP: 8, LDS_LARGE: 8, GLOBAL: 16, LANE: 5, WAVE: 8, LANE_REG: 8, WIDE: None, WIDE_HBM: None}
# Deps per Add a tier reads: the tier table's max_deps (graph_tiers.hip:42-73): GROUP_LANES, MAX_DEPS,
# WAVE_MAX_DEPS, LANE_MAX_DEPS.
MAX_DEPS = {GROUP: 16, LDS_LARGE: 31, GLOBAL: 31, LANE: 31, WAVE: 14, LANE_REG: 8, SPLIT: 16, WIDE: 31, WIDE_HBM: 31}
# The ladder: TierDesc::next (graph_tiers.hip:42-73).
NEXT = {GROUP: LDS_LARGE, LDS_LARGE: GLOBAL, GLOBAL: WIDE, LANE: LDS_LARGE, WAVE: GLOBAL, LANE_REG: LDS_LARGE,
        SPLIT: LDS_LARGE, WIDE: WIDE_HBM, WIDE_HBM: None}
WIDE_INDEX = 256  # index slots per source of the LDS wide tier (graph_wide.hip:840)

# P pending, C cached deps (None: no limit), W window bits, WLC worklist entries, Q index slots per source (None:
# not a limit), wide: every Add takes a vertex and SCCs reach the clock in pop order, masks: the worklist holds
# LANE_REG's waiter masks
Limits = collections.namedtuple("Limits", "P C W WLC Q wide masks")


def tier_limits(tier, n):
    """A tier's table sizes: pending_cap and window_bits from fx_tier_query, the rest restated."""
    info = _lib.TierInfo()
    _lib.check(_lib.load().fx_tier_query(tier, n, ctypes.byref(info)), "fx_tier_query")
    P, W = int(info.pending_cap), int(info.window_bits)
    wide = tier in (WIDE, WIDE_HBM)
    # worklist: WLC = P + 1 (graph_group.hip:35, graph_wave.hip:37, graph_exec.hip:68), P + 2 masks
    # (graph_lane.hip:61), wlcap = P packed and 2 P in HBM (graph_wide.hip:86)
    wlc = {LANE_REG: P + 2, WIDE: P, WIDE_HBM: 2 * P}.get(tier, P + 1)
    return Limits(P, CACHE[tier], W, wlc, WIDE_INDEX if tier == WIDE else None, wide, tier == LANE_REG)


class Stop(Exception):
    def __init__(self, resource):
        Exception.__init__(self, resource)
        self.resource = resource


class Vertex:
    __slots__ = ("rec", "deps", "wait")

    def __init__(self, rec, deps):
        self.rec, self.deps, self.wait = rec, deps, None


class Graph:
    def __init__(self, n, lim=None, init_frontier=None):
        self.n, self.lim = n, lim
        self.front = [0] * (n + 1)
        if init_frontier is not None:
            self.front[1:] = [int(f) for f in init_frontier[:n]]
        self.exs = [set() for _ in range(n + 1)]
        self.top = [0] * (n + 1)  # highest seq executed
        self.pend = {}
        self.waiting = collections.defaultdict(set)  # missing dot -> the dots registered on it (PendingIndex)
        self.shared = collections.Counter()          # (source, seq mod WIDE_INDEX) of the pending dots
        self.order, self.release = [], {}
        self.cur = 0
        self.wl = []  # check_pending's worklist: [dot, had waiters when it executed]
        self.stats = dict(slots=0, slots_all=0, cache=0, off=-1, off_pop=-1, wl=0, wl_mask=0, index=False,
                          max_pending=0, max_window=0)

    # ------------------------------------------------------------ executed clock
    def contains(self, d):
        s, q = d
        return 1 <= s <= self.n and (q <= self.front[s] or q in self.exs[s])

    def clk_add(self, d, names=("off",)):
        """AEClock::add; counts seq - frontier - 1 under each of `names`."""
        s, q = d
        f = self.front[s]
        if q <= f:
            return
        off = q - f - 1
        for name in names:
            self.stats[name] = max(self.stats[name], off)
        if self.lim is not None and ("off_pop" if self.lim.wide else "off") in names and off >= self.lim.W:
            raise Stop("window")
        self.exs[s].add(q)
        self.top[s] = max(self.top[s], q)
        while f + 1 in self.exs[s]:
            f += 1
            self.exs[s].discard(f)
        self.front[s] = f

    def count_pop_order(self, members):
        """The offsets an SCC's members meet when they reach the clock in pop order (last pushed first)."""
        if len(members) == 1:  # a singleton meets what the ascending order meets
            s, q = members[0]
            if q > self.front[s]:
                self.stats["off_pop"] = max(self.stats["off_pop"], q - self.front[s] - 1)
                if self.lim is not None and self.lim.wide and q - self.front[s] - 1 >= self.lim.W:
                    raise Stop("window")
            return
        saved = self.front[:], [set(e) for e in self.exs], self.top[:]
        try:
            for d in reversed(members):
                self.clk_add(d, ("off_pop",))
        finally:
            self.front, self.exs, self.top = saved

    # ------------------------------------------------------------ vertex index
    def waiters(self, x):
        return sorted(self.waiting.get(x, ()))

    def register(self, d, missing):
        """index_pending / PendingIndex::remove for one waiter (missing None: no longer registered)."""
        v = self.pend[d]
        if v.wait is not None:
            self.waiting[v.wait].discard(d)
            if not self.waiting[v.wait]:
                del self.waiting[v.wait]
        v.wait = missing
        if missing is not None:
            self.waiting[missing].add(d)

    def remove(self, d):
        self.register(d, None)
        self.shared[(d[0], d[1] % WIDE_INDEX)] -= 1
        del self.pend[d]

    def insert(self, rec, d, kept):
        st = self.stats
        st["slots"] = max(st["slots"], len(self.pend) + 1)
        if self.lim is not None and not self.lim.wide and len(self.pend) + 1 > self.lim.P:
            raise Stop("slots")
        st["cache"] = max(st["cache"], len(kept))
        if self.lim is not None and self.lim.C is not None and len(kept) > self.lim.C:
            raise Stop("cache")
        self.pend[d] = Vertex(rec, kept)
        self.shared[(d[0], d[1] % WIDE_INDEX)] += 1

    def push(self, dots, fast=False):
        """The executed dots of one SCC (or the fast path's dot) onto the worklist.  A dot's flag: something was
        registered on it when it executed, the SCC's members still in the index as LANE_REG has them then
        (graph_lane.hip:449, :521-524); the fast path's dot is no entry of LANE_REG's."""
        st = self.stats
        for d in dots:
            self.wl.append([d, not fast and bool(self.waiters(d))])
        masks = sum(1 for _, w in self.wl if w)
        st["wl"] = max(st["wl"], len(self.wl))
        st["wl_mask"] = max(st["wl_mask"], masks)
        if self.lim is not None and (masks if self.lim.masks else len(self.wl)) > self.lim.WLC:
            raise Stop("worklist")

    # ------------------------------------------------------------ find_scc
    def save_scc(self, members):
        """save_scc: members (in Tarjan-stack order) to to_execute and the executed clock, ascending by dot."""
        self.count_pop_order(members)
        members = sorted(members)
        for i, d in enumerate(members):
            v = self.pend[d]
            self.order.append((v.rec, i == 0))
            self.release[v.rec] = self.cur
            self.clk_add(d)
        self.push(members)
        for d in members:
            self.remove(d)

    def find_scc(self, root):
        """strong_connect from root, iteratively; returns (missing dot or None, an SCC was saved, the dots left on
        the Tarjan stack)."""
        ids, low, stack = {root: 1}, {root: 1}, [root]
        frames, idc, saved = [[root, 0]], 1, False
        while frames:
            v, i = frames[-1]
            deps = self.pend[v].deps
            if i < len(deps):
                frames[-1][1] = i + 1
                dep = deps[i]
                if self.contains(dep):
                    continue
                if dep not in self.pend:
                    return dep, saved, stack
                if dep not in ids:
                    idc += 1
                    ids[dep] = low[dep] = idc
                    stack.append(dep)
                    frames.append([dep, 0])
                else:  # visited: on the stack (a saved vertex is executed, and was skipped above)
                    low[v] = min(low[v], ids[dep])
                continue
            if ids[v] == low[v]:
                pos = stack.index(v)
                members = stack[pos:]
                del stack[pos:]
                self.save_scc(members)
                for m in members:
                    del ids[m]
                saved = True
            frames.pop()
            if frames:
                p = frames[-1][0]
                low[p] = min(low[p], low[v])
        return None, saved, stack

    # ------------------------------------------------------------ check_pending / try_pending
    def check_pending(self):
        while self.wl:
            x = self.wl.pop()[0]
            ws = self.waiters(x)
            for d in ws:
                self.register(d, None)
            visited = set()
            for d in ws:
                if d not in self.pend or d in visited:  # executed meanwhile; visited: skipped, not re-registered
                    continue
                missing, saved, left = self.find_scc(d)
                if missing is not None and not saved:
                    visited.update(left)
                else:
                    visited.clear()
                if missing is not None:
                    self.register(d, missing)

    # ------------------------------------------------------------ handle_add
    def handle_add(self, i, d, deps, kind):
        st, lim = self.stats, self.lim
        self.cur, self.wl = i, []
        if not (1 <= d[0] <= self.n) or d[1] == 0:
            return FX_ERR_DOT_RANGE
        if d in self.pend:
            return FX_ERR_DOUBLE_INDEX
        st["slots_all"] = max(st["slots_all"], len(self.pend) + 1)
        if self.shared[(d[0], d[1] % WIDE_INDEX)] > 0:
            st["index"] = True
            if lim is not None and lim.Q:
                raise Stop("index")
        if lim is not None and lim.wide and len(self.pend) + 1 > lim.P:
            raise Stop("slots")
        kept = [x for x in sorted(set(deps)) if x != d and not self.contains(x)]
        if kind == _lib.FX_KIND_INDEX_ONLY:
            self.insert(i, d, kept)
            return 0
        if not kept:  # every dep is the dot itself or executed: a singleton SCC
            self.order.append((i, True))
            self.release[i] = i
            self.clk_add(d, ("off", "off_pop"))
            if self.waiting:
                self.push([d], fast=True)
            self.check_pending()
            return 0
        self.insert(i, d, kept)
        missing, _, _ = self.find_scc(d)
        if missing is not None:
            self.register(d, missing)
        self.check_pending()
        return 0


def run(stream, n, lim=None, init_frontier=None):
    """Runs a stream; lim: a tier's Limits (None: unbounded).  Returns order [(arrival, scc_start)], release
    {arrival: step}, pending (arrivals left pending), nexec, err, row (where it stopped, None: at its end),
    stop (the resource that stopped it), stats."""
    g = Graph(n, lim, init_frontier)
    err, row, stop = 0, None, None
    for i, add in enumerate(stream):
        d, deps = tuple(add[0]), [tuple(x) for x in add[1]]
        kind = add[3] if len(add) > 3 else _lib.FX_KIND_ADD
        try:
            err = g.handle_add(i, d, deps, kind)
        except Stop as e:
            err, stop = FX_ERR_CAPACITY, e.resource
        if err:
            row = i
            break
        g.stats["max_pending"] = max(g.stats["max_pending"], len(g.pend))
        for s in range(1, n + 1):
            if g.exs[s]:
                g.stats["max_window"] = max(g.stats["max_window"], g.top[s] - g.front[s])
    return dict(order=g.order, release=g.release, pending=sorted(v.rec for v in g.pend.values()),
                nexec=len(g.order), err=err, row=row, stop=stop, stats=g.stats)


def exceeded(stats, lim):
    """The resources of `lim` a stream with these counters outgrows."""
    out = []
    if (stats["slots_all"] if lim.wide else stats["slots"]) > lim.P:
        out.append("slots")
    if lim.C is not None and stats["cache"] > lim.C:
        out.append("cache")
    if (stats["off_pop"] if lim.wide else stats["off"]) >= lim.W:
        out.append("window")
    if (stats["wl_mask"] if lim.masks else stats["wl"]) > lim.WLC:
        out.append("worklist")
    if lim.Q and stats["index"]:
        out.append("index")
    return out


def fits(stats, tier, n):
    """Whether a stream with these counters (of an unbounded run) stays within a tier's tables."""
    return not exceeded(stats, tier_limits(tier, n))
