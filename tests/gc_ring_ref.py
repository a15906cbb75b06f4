"""A plain-Python restatement of the GC track of the all-on-chip simulator
(k_sim, sim_wave.hip): the ring of a pair's last frontier moves (h_mcommitdot),
the time query on it (gc_value_at) and the Stable counts evaluated from the
rings at the end of a run (gc_finish); and, beside it, the same Stable counts
by brute force: every GC delivery enumerated, every look-up over the full
history of moves.  tests/test_sim_gc_ring_ref.py sets the two against each
other; tests/test_sim_gc_ring.py uses them to pick instances whose rings lose
an entry.

A history is the list of a pair's moves in order, (time, frontier after the
move), times ascending (several moves may share a millisecond).  d[p][q] is the
link delay p -> q in ms, gc the GC interval; tick k of p fires at (k + 1) gc,
after the other actions of its millisecond, and reaches q at (k + 1) gc +
d[p][q].  A run that ends at time tc has processed the GC actions before tc,
plus the delivery `pair` = (p, q) at tc if it stopped on it.
"""

RD_BASE = 6  # entries per client per region (geo_make)


def ring_depth(n, clients, wslots=0):
    """Geo::rd of a launch of n processes and `clients` clients (wslots: the
    dot-table slots asked for; more than 64 is the rerun geometry)."""
    cpr = (clients + n - 1) // n
    rd = RD_BASE
    while rd < RD_BASE * cpr and rd < 96:
        rd *= 2
    w = wslots if wslots else (32 if n > 5 and clients <= 8 else min(64, 8 * clients))
    return max(rd, 48) if w > 64 else rd


class Ring:
    """The kernel's ring of one pair: move c goes to entry c mod depth."""

    def __init__(self, depth):
        self.depth = depth
        self.entries = [None] * depth  # a word read before it was written would show as None
        self.count = 0

    def move(self, now, frontier):
        self.entries[self.count % self.depth] = (now, frontier)
        self.count += 1

    def value_at(self, x):
        """(ok, frontier after every move up to time x): the newest entry with
        time <= x; 0 before the first move if the ring never wrapped; not ok
        if the ring has lost the answer."""
        e = self.count % self.depth
        for _ in range(min(self.count, self.depth)):
            e = (e if e else self.depth) - 1
            if self.entries[e][0] <= x:
                return True, self.entries[e][1]
        return self.count <= self.depth, 0


def ring_of(history, depth):
    r = Ring(depth)
    for t, f in history:
        r.move(t, f)
    return r


def full_value_at(history, x):
    """(index of the answering move or -1, frontier) over the whole history."""
    j, v = -1, 0
    for i, (t, f) in enumerate(history):
        if t <= x:
            j, v = i, f
    return j, v


def overwritten(history, x, depth):
    """Whether a ring of `depth` entries has overwritten what the query at x
    needs: the answering move, or the first move where the answer is that
    nothing moved yet (only the first move still in place proves that)."""
    j, _ = full_value_at(history, x)
    return max(j, 0) < len(history) - depth


def finish_ring(n, rings, d, gc, tc, pair=None):
    """gc_finish: (ok, Stable count per process) from rings[p][s]."""
    ok, out = True, []
    for q in range(n):
        m = [0] * n
        for p in range(n):
            if p == q:
                continue
            if tc > d[p][q]:
                m[p] = (tc - d[p][q] - 1) // gc
            if pair == (p, q) and tc >= d[p][q] + gc and (tc - d[p][q]) % gc == 0:
                m[p] += 1
        if any(m[p] == 0 for p in range(n) if p != q):
            out.append(0)
            continue
        tl = max(m[p] * gc + d[p][q] for p in range(n) if p != q)
        stable = 0
        for s in range(n):
            o, cur = rings[q][s].value_at(tl)
            ok = ok and o
            for p in range(n):
                if p != q:
                    o, v = rings[p][s].value_at(m[p] * gc)
                    ok = ok and o
                    cur = min(cur, v)
            stable += cur
        out.append(stable)
    return ok, out


def finish_brute(n, hist, d, gc, tc, pair=None, depth=None):
    """The same Stable counts from the enumerated GC deliveries and the full
    histories hist[p][s]; with `depth`, also whether a ring of that depth has
    overwritten an entry some look-up needs: (lost, counts)."""
    lost, out = False, []
    for q in range(n):
        last = {}  # p -> time of the newest tick of p delivered to q
        tl = 0
        for p in range(n):
            if p == q:
                continue
            k = 0
            while True:
                fire = (k + 1) * gc
                at = fire + d[p][q]
                if not (at < tc or (at == tc and pair == (p, q))):
                    break
                last[p] = fire
                tl = max(tl, at)
                k += 1
        if len(last) < n - 1:
            out.append(0)
            continue
        stable = 0
        for s in range(n):
            looks = [(hist[q][s], tl)] + [(hist[p][s], last[p]) for p in sorted(last)]
            stable += min(full_value_at(h, x)[1] for h, x in looks)
            if depth is not None:
                lost = lost or any(overwritten(h, x, depth) for h, x in looks)
        out.append(stable)
    return lost, out


def histories_from_adds(n, streams):
    """hist[p][s] from each process's commits in handle order, streams[p] =
    [((source, seq), deps, t_ms)] (oracle_lib.sim_capture): the committed clock
    of source s + 1 at p is a frontier plus the seqs above it (gc/clock.rs),
    and a move is a commit that raises the frontier."""
    hist = [[[] for _ in range(n)] for _ in range(n)]
    for p in range(n):
        front = [0] * n
        above = [set() for _ in range(n)]
        for (src, seq), _deps, t in streams[p]:
            s = src - 1
            if seq <= front[s]:
                continue
            above[s].add(seq)
            if seq == front[s] + 1:
                while front[s] + 1 in above[s]:
                    front[s] += 1
                    above[s].remove(front[s])
                hist[p][s].append((t, front[s]))
    return hist
