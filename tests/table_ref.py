"""CPU restatement of Tempo's TableExecutor for single-key commands and
shard_count = 1, in plain Python: what the GPU table executor (fx_table_*) is
compared against, bit for bit.  Cited lines are the reference's
fantoch_ps/src/executor/table/mod.rs unless another file is named.

Where the reference panics, run_stream stops the stream at that event with
the status the GPU reports; the event leaves the votes tables as they were.
"""
FX_OK = 0
FX_ERR_INVALID_ARG = 1
FX_ERR_DOUBLE_INDEX = 3
FX_ERR_DOT_RANGE = 5
FX_ERR_VOTE_RANGE = 16
SEQ_MASK = (1 << 24) - 1


class VoteError(Exception):
    pass


class EventSet:
    """One process's votes on one key: every vote 1..frontier was seen, plus
    the votes in `above` (the event set inside the ARClock of :112,127-128)."""

    def __init__(self):
        self.frontier = 0
        self.above = set()

    def add_range(self, start, end):
        """Adds start..end; True if at least one vote was new (:180).  A range
        that starts at the frontier costs the votes held above, not its
        length: the frontier moves to `end` and the votes at or below it go."""
        if end <= self.frontier:
            return False
        if start <= self.frontier + 1:
            seen = [v for v in self.above if v <= end]
            new = len(seen) < end - self.frontier
            self.above.difference_update(seen)
            self.frontier = end
        else:
            fresh = [v for v in range(start, end + 1) if v not in self.above]
            self.above.update(fresh)
            new = bool(fresh)
        while self.frontier + 1 in self.above:
            self.frontier += 1
            self.above.remove(self.frontier)
        return new

    def copy(self):
        c = EventSet()
        c.frontier, c.above = self.frontier, set(self.above)
        return c


class VotesTable:
    """:104-267."""

    def __init__(self, n, stability_threshold):
        self.n, self.thr = n, stability_threshold
        self.clock = {p: EventSet() for p in range(1, n + 1)}  # :127-128
        self.ops = {}  # (clock, dot) -> pending; kept sorted on demand (:116)
        self.max_above = 0  # how far above a frontier a vote was added (tier capacities)

    def add_votes(self, votes):
        """add_detached_votes (:171-194); raises VoteError and changes nothing
        when a range is malformed (votes.rs:111) or adds no new vote (:180)."""
        work = {}
        for voter, start, end in votes:
            if not 1 <= voter <= self.n or start == 0 or start > end:
                raise VoteError()
            es = work.get(voter) or self.clock[voter].copy()
            work[voter] = es
            above = end - es.frontier
            if not es.add_range(start, end):
                raise VoteError()
            self.max_above = max(self.max_above, above)
        self.clock.update(work)

    def stable_clock(self):
        """:243-266: index n - threshold of the frontiers sorted ascending."""
        return sorted(es.frontier for es in self.clock.values())[self.n - self.thr]

    def stable_ops(self):
        """:196-240: the ops with clock <= stable clock leave, ascending by
        (clock, dot).  split_off's bound (stable + 1, Dot(1, 1)) is excluded
        and no dot sorts below (1, 1)."""
        stable = self.stable_clock()
        ids = sorted(sid for sid in self.ops if sid[0] <= stable)
        return [self.ops.pop(sid) for sid in ids]


def run_stream(events, n, stability_threshold, keys, vmax=None, execute_at_commit=False):
    """One executor's stream (executor.rs:110-144).  Returns a dict: order
    (arrival indices as executed), release {arrival: step}, nexec, err,
    stable (stable clock per key after the last processed event, 0 for a key
    never seen), steps (the ids executed by each processed event),
    max_pending and max_above (what the stream asks of a GPU tier)."""
    tables = {}
    order, release, steps = [], {}, []
    err, max_pending, pending = FX_OK, 0, 0
    for r, ev in enumerate(events):
        kind, key, votes = ev[0], ev[1], ev[-1]
        if key >= keys or (vmax is not None and len(votes) > vmax):
            err = FX_ERR_INVALID_ARG
            break
        if kind == "A":
            (src, seq), clock = ev[2], ev[3]
            if not 1 <= src <= n or not 1 <= seq <= SEQ_MASK:
                err = FX_ERR_DOT_RANGE
                break
            if execute_at_commit:  # executor.rs:125-126
                order.append(r)
                release[r] = r
                steps.append([r])
                continue
        elif execute_at_commit:  # executor.rs:134-139
            steps.append([])
            continue
        table = tables.get(key)
        if table is None:  # :85-98
            table = tables[key] = VotesTable(n, stability_threshold)
        if kind == "A":
            sid = (clock, (src, seq))  # :151
            if sid in table.ops:  # :163-165
                err = FX_ERR_DOUBLE_INDEX
                break
            table.ops[sid] = r
            pending += 1
            max_pending = max(max_pending, pending)
        try:
            table.add_votes(votes)
        except VoteError:
            err = FX_ERR_VOTE_RANGE
            break
        done = table.stable_ops()
        for a in done:
            order.append(a)
            release[a] = r
        pending -= len(done)
        steps.append(done)
    stable = [tables[k].stable_clock() if k in tables else 0 for k in range(keys)]
    return dict(order=order, release=release, nexec=len(order), err=err, stable=stable, steps=steps,
                max_pending=max_pending, max_above=max([t.max_above for t in tables.values()] + [0]))
