"""CPU restatement of Tempo's TableExecutor with multi-key commands and the
StableAtShard messages an executor sends itself (shard_count = 1), in plain
Python over the votes tables of tests/table_ref.py: what fx_table_execute_mk /
fx_table_run_mk are compared against, bit for bit.  Cited lines are the
reference's fantoch_ps/src/executor/table/executor.rs unless another file is
named.

An attached event is ("A", key, dot, clock, votes[, nkeys]): one AttachedVotes
of a command with nkeys keys (1 when absent), all on this shard, so
missing_stable_shards starts at 1 and shard_key_count is nkeys (:57-61).  The
rifl of a command is its dot.  Tempo emits the nkeys events of a command with
the same dot and clock (fantoch_ps/src/protocol/tempo.rs:614-636).

What the reference leaves open and this file fixes (DESIGN.md section 1.1,
C13): the keys of a command receive their StableAtShard in ascending key id
(pushed in that order, so popped in descending order); the other keys of a
command are the keys of its partials that tried and wait (with the checked
input contract below: every other key of the command).

Input contract, checked when an attached event arrives against the partials
of the same dot that have not executed yet: same nkeys, same clock, another
key, fewer than nkeys of them, and none already told that the command is
stable at the shard.  A violation stops the stream with FX_ERR_INVALID_ARG.
Events of a dot whose earlier partials have all executed cannot be told from
a new command and start one.
"""
from table_ref import (FX_ERR_DOT_RANGE, FX_ERR_DOUBLE_INDEX, FX_ERR_INVALID_ARG, FX_ERR_VOTE_RANGE, FX_OK, SEQ_MASK,
                       VoteError, VotesTable)

MAX_CMD_KEYS = 8  # FX_TABLE_MAX_CMD_KEYS


class VotesTableMk(VotesTable):
    """VotesTable that also records max_gap_above: how far above a frontier a
    vote was added by a range that did not start at the frontier (a range that
    does only moves the frontier, whatever its length: what the _mk ONCHIP
    tier asks of its window)."""

    def __init__(self, n, stability_threshold):
        super().__init__(n, stability_threshold)
        self.max_gap_above = 0

    def add_votes(self, votes):
        work, gap = {}, 0  # the ranges in order, on copies, as super().add_votes applies them
        for voter, start, end in votes:
            if not 1 <= voter <= self.n or start == 0 or start > end:
                break
            es = work.get(voter) or self.clock[voter].copy()
            work[voter] = es
            if start > es.frontier + 1:
                gap = max(gap, end - es.frontier)
            if not es.add_range(start, end):
                break
        super().add_votes(votes)  # raises and changes nothing on a bad range
        self.max_gap_above = max(self.max_gap_above, gap)


class Pending:
    """Pending (:40-76) of one (command, key) partial."""

    def __init__(self, arrival, key, dot, clock, nkeys):
        self.arrival, self.key, self.dot, self.clock = arrival, key, dot, clock
        self.shard_key_count = nkeys  # :57-60
        self.missing_stable_shards = 1  # :61, one shard
        self.told = False  # a StableAtShard for it is on its way (only the input check reads this)

    def single_key_command(self):
        return self.missing_stable_shards == 1 and self.shard_key_count == 1  # :71-75


class Executor:
    """TableExecutor (:20-31) plus the runner's drain (fantoch/src/sim/runner.rs:405-419)."""

    def __init__(self, n, stability_threshold):
        self.n, self.thr = n, stability_threshold
        self.tables = {}
        self.pending = {}  # key -> list of Pending, the VecDeque of :35
        self.buffered = {}  # key -> {dot: count}, stable_shards_buffered of :36
        self.count = {}  # dot -> partials that tried, rifl_to_stable_count of :30
        self.tried = {}  # dot -> the Pendings counted in self.count[dot]
        self.to_executors = []  # :28
        self.live = {}  # dot -> partials not executed yet (the input check)
        self.nlive = 0
        self.order, self.release = [], {}
        self.step = 0
        self.max_live = self.max_stack = self.buffered_msgs = 0

    # :365-380
    def do_execute(self, p):
        self.order.append(p.arrival)
        self.release[p.arrival] = self.step
        self.live[p.dot].remove(p)
        if not self.live[p.dot]:
            del self.live[p.dot]
        self.nlive -= 1

    def push(self, key, dot):
        self.to_executors.append((key, dot))

    # :280-359; True when the op executed, False when it is handed back
    def try_op(self, p):
        if p.single_key_command():  # :290-293
            self.do_execute(p)
            return True
        # shard_key_count > 1 here (:311 is the case of other shards)
        self.count[p.dot] = self.count.get(p.dot, 0) + 1  # :319-322
        self.tried.setdefault(p.dot, []).append(p)
        if self.count[p.dot] == p.shard_key_count:  # :328
            # send_stable_msg (:296-309): every other key, ascending (C13)
            for q in sorted((q for q in self.tried[p.dot] if q is not p), key=lambda q: q.key):
                q.told = True
                self.push(q.key, p.dot)
            p.missing_stable_shards -= 1  # :333
            del self.count[p.dot]  # :338-340
            del self.tried[p.dot]
        c = self.buffered.get(p.key, {}).pop(p.dot, None)  # :345-347
        if c is not None:
            p.missing_stable_shards = (p.missing_stable_shards - c) & 0xFFFFFFFF
        if p.missing_stable_shards == 0:  # :349-352
            self.do_execute(p)
            return True
        return False  # :353-357

    # :237-277
    def send_stable_or_execute(self, key, to_execute):
        q = self.pending.setdefault(key, [])
        if q:  # :242-247
            q.extend(to_execute)
            return
        for i, p in enumerate(to_execute):  # :250-276
            if not self.try_op(p):
                q.append(p)
                q.extend(to_execute[i + 1:])
                return

    # :168-235
    def handle_stable_msg(self, key, dot):
        q = self.pending.setdefault(key, [])
        if q and q[0].dot == dot:  # :173-175
            q[0].missing_stable_shards -= 1  # :177
            if q[0].missing_stable_shards == 0:  # :186-195
                self.do_execute(q.pop(0))
                while q:  # :198-217
                    p = q.pop(0)
                    if not self.try_op(p):
                        q.insert(0, p)
                        return
        else:  # :219-233
            b = self.buffered.setdefault(key, {})
            b[dot] = b.get(dot, 0) + 1
            self.buffered_msgs += 1

    def drain(self):
        """runner.rs:411-416: pop until empty (LIFO), then handle each once;
        what the handlers push waits for the next event."""
        msgs = []
        while self.to_executors:
            msgs.append(self.to_executors.pop())
        for i, (key, dot) in enumerate(msgs):
            self.handle_stable_msg(key, dot)
            # the collected messages not handled yet and the new ones are held together
            self.max_stack = max(self.max_stack, len(msgs) - i - 1 + len(self.to_executors))


def run_stream(events, n, stability_threshold, keys, vmax=None, execute_at_commit=False):
    """One executor's stream.  Returns what table_ref.run_stream returns
    (order, release, nexec, err, stable, max_above) with one order row and one
    release entry per executed (command, key) partial, and: max_live (the most
    partials that arrived and had not executed: votes tables plus queues),
    max_stack (the deepest to_executors, counting the collected messages of a
    drain until each is handled), buffered (StableAtShard messages buffered),
    unhandled (messages left in to_executors after the last event),
    max_gap_above (VotesTableMk)."""
    ex = Executor(n, stability_threshold)
    err = FX_OK
    for r, ev in enumerate(events):
        ex.step = r
        kind, key = ev[0], ev[1]
        votes = ev[4] if kind == "A" else ev[2]
        if key >= keys or (vmax is not None and len(votes) > vmax):
            err = FX_ERR_INVALID_ARG
            break
        if kind == "A":
            (src, seq), clock = ev[2], ev[3]
            nkeys = ev[5] if len(ev) > 5 else 1
            if not 1 <= nkeys <= MAX_CMD_KEYS:
                err = FX_ERR_INVALID_ARG
                break
            if not 1 <= src <= n or not 1 <= seq <= SEQ_MASK:
                err = FX_ERR_DOT_RANGE
                break
            if execute_at_commit:  # :125-126
                ex.order.append(r)
                ex.release[r] = r
                continue
        elif execute_at_commit:  # :134-139
            continue
        table = ex.tables.get(key)
        if table is None:
            table = ex.tables[key] = VotesTableMk(n, stability_threshold)
        if kind == "A":
            dot = (src, seq)
            if (clock, dot) in table.ops:  # mod.rs:163-165
                err = FX_ERR_DOUBLE_INDEX
                break
            mates = ex.live.get(dot, [])
            if len(mates) >= nkeys or any(q.shard_key_count != nkeys or q.clock != clock or q.key == key or q.told
                                          for q in mates):
                err = FX_ERR_INVALID_ARG
                break
            p = Pending(r, key, dot, clock, nkeys)
            table.ops[(clock, dot)] = p
            ex.live.setdefault(dot, []).append(p)
            ex.nlive += 1
            ex.max_live = max(ex.max_live, ex.nlive)
        try:
            table.add_votes(votes)
        except VoteError:
            err = FX_ERR_VOTE_RANGE
            if kind == "A":  # the event leaves no trace
                del table.ops[(clock, dot)]
                ex.live[dot].remove(p)
                ex.nlive -= 1
            break
        ex.send_stable_or_execute(key, table.stable_ops())
        ex.max_stack = max(ex.max_stack, len(ex.to_executors))
        ex.drain()
    stable = [ex.tables[k].stable_clock() if k in ex.tables else 0 for k in range(keys)]
    return dict(order=ex.order, release=ex.release, nexec=len(ex.order), err=err, stable=stable,
                max_live=ex.max_live, max_stack=ex.max_stack, buffered=ex.buffered_msgs,
                unhandled=len(ex.to_executors), max_above=max([t.max_above for t in ex.tables.values()] + [0]),
                max_gap_above=max([t.max_gap_above for t in ex.tables.values()] + [0]))
