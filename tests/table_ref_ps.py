"""CPU restatement of Tempo's TableExecutor for commands that span shards
(shard_count > 1): tests/table_ref_mk.py's Executor with the rest of the
reference's fantoch_ps/src/executor/table/executor.rs -- missing_stable_shards
that starts at the command's shard count (:61), the send of a command with
one key at this shard (:311-316), StableAtShard messages from other shards
(:140-142, :168-235) and the buffered counts (:219-233, :345-347).  What
fx_table_execute_ps / fx_table_run_ps are compared against, bit for bit.
Cited lines are executor.rs unless another file is named.

Events: ("A", key, dot, clock, votes[, nkeys[, shards]]) -- nkeys the
command's keys at this shard, shards the shards it accesses, this one
included, both 1 when absent -- ("D", key, votes) and ("S", key, dot), a
StableAtShard{key, rifl} another shard's executor sent (the rifl is the dot).

The reference has no executor-level test with shard_count > 1, so this file is
the pin.  Beside what table_ref_mk.py fixes:
  * a buffered count above missing_stable_shards, where the reference's usize
    would underflow, stops the stream with FX_ERR_INVALID_ARG before anything
    of that try is recorded (what the same event executed before it stays);
  * the partial that ran send_stable_msg counts as told in the input check,
    which also asks for the same `shards` on every event of a dot;
  * not caught: a message beyond the shards - 1 that other shards can send,
    for a head whose own shard is not stable yet, executes it early.
"""
import table_ref_mk as RM
from table_ref import (FX_ERR_DOT_RANGE, FX_ERR_DOUBLE_INDEX, FX_ERR_INVALID_ARG, FX_ERR_VOTE_RANGE, FX_OK, SEQ_MASK,
                       VoteError)

MAX_CMD_KEYS = RM.MAX_CMD_KEYS
MAX_CMD_SHARDS = 8  # FX_TABLE_MAX_CMD_SHARDS


class CountError(Exception):
    """A buffered count above missing_stable_shards (:346 would underflow)."""


class Pending(RM.Pending):
    def __init__(self, arrival, key, dot, clock, nkeys, shards):
        super().__init__(arrival, key, dot, clock, nkeys)
        self.shards = shards
        self.missing_stable_shards = shards  # :61


class Executor(RM.Executor):
    def __init__(self, n, stability_threshold):
        super().__init__(n, stability_threshold)
        self.sent = {}  # arrival -> the step during which that partial ran send_stable_msg
        self.npairs = self.max_buffered_pairs = self.max_count = 0

    # :280-359; True when the op executed, False when it is handed back
    def try_op(self, p):
        if p.single_key_command():  # :290-293 (:71-75: one shard and one key there)
            self.do_execute(p)
            return True
        sends = False
        if p.shard_key_count == 1:  # :311-316: no other key at this shard to tell
            sends = True
        else:
            self.count[p.dot] = self.count.get(p.dot, 0) + 1  # :319-322
            self.tried.setdefault(p.dot, []).append(p)
            if self.count[p.dot] == p.shard_key_count:  # :328
                # send_stable_msg (:296-309), the keys at this shard: every other one, ascending (C13)
                for q in sorted((q for q in self.tried[p.dot] if q is not p), key=lambda q: q.key):
                    q.told = True
                    self.push(q.key, p.dot)
                sends = True
                del self.count[p.dot]  # :338-340
                del self.tried[p.dot]
        missing = p.missing_stable_shards - (1 if sends else 0)  # :316, :333
        c = self.buffered.get(p.key, {}).get(p.dot)  # :345-347
        if c is not None:
            if c > missing:
                raise CountError()
            del self.buffered[p.key][p.dot]
            self.npairs -= 1
            missing -= c
        p.missing_stable_shards = missing
        if sends:
            p.told = True
            self.sent[p.arrival] = self.step
        if missing == 0:  # :349-352
            self.do_execute(p)
            return True
        return False  # :353-357

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
        else:  # :219-233: the queue is empty or its head is another command
            b = self.buffered.setdefault(key, {})
            if dot not in b:
                self.npairs += 1
                self.max_buffered_pairs = max(self.max_buffered_pairs, self.npairs)
            b[dot] = b.get(dot, 0) + 1
            self.max_count = max(self.max_count, b[dot])
            self.buffered_msgs += 1


class Stream:
    """One executor fed event by event (the co-simulation of a group of shard
    executors needs what an event sent before the next is chosen)."""

    def __init__(self, n, stability_threshold, keys, vmax=None, execute_at_commit=False):
        self.ex = Executor(n, stability_threshold)
        self.n, self.keys, self.vmax, self.at_commit = n, keys, vmax, execute_at_commit
        self.err = FX_OK
        self.r = 0

    def feed(self, ev):
        """Handles the next event and the drain after it; returns the status
        (a stream that failed handles nothing more)."""
        if self.err == FX_OK:
            self.ex.step = self.r
            self.err = self._handle(self.r, ev)
            self.r += 1
        return self.err

    def _handle(self, r, ev):
        ex, n = self.ex, self.n
        kind, key = ev[0], ev[1]
        if kind == "S":  # :140-142
            src, seq = ev[2]
            if key >= self.keys:
                return FX_ERR_INVALID_ARG
            if not 1 <= src <= n or not 1 <= seq <= SEQ_MASK:
                return FX_ERR_DOT_RANGE
            if self.at_commit:
                return FX_OK
            try:
                ex.handle_stable_msg(key, (src, seq))
                ex.max_stack = max(ex.max_stack, len(ex.to_executors))
                ex.drain()
            except CountError:
                return FX_ERR_INVALID_ARG
            return FX_OK
        votes = ev[4] if kind == "A" else ev[2]
        if key >= self.keys or (self.vmax is not None and len(votes) > self.vmax):
            return FX_ERR_INVALID_ARG
        if kind == "A":
            (src, seq), clock = ev[2], ev[3]
            nkeys = ev[5] if len(ev) > 5 else 1
            shards = ev[6] if len(ev) > 6 else 1
            if not 1 <= shards <= MAX_CMD_SHARDS or not 1 <= nkeys <= MAX_CMD_KEYS:
                return FX_ERR_INVALID_ARG
            if not 1 <= src <= n or not 1 <= seq <= SEQ_MASK:
                return FX_ERR_DOT_RANGE
            if self.at_commit:  # :125-126
                ex.order.append(r)
                ex.release[r] = r
                return FX_OK
        elif self.at_commit:  # :134-139
            return FX_OK
        table = ex.tables.get(key)
        if table is None:
            table = ex.tables[key] = RM.VotesTableMk(n, ex.thr)
        if kind == "A":
            dot = (src, seq)
            if (clock, dot) in table.ops:  # mod.rs:163-165
                return FX_ERR_DOUBLE_INDEX
            mates = ex.live.get(dot, [])
            if len(mates) >= nkeys or any(q.shard_key_count != nkeys or q.shards != shards or q.clock != clock or
                                          q.key == key or q.told for q in mates):
                return FX_ERR_INVALID_ARG
            p = Pending(r, key, dot, clock, nkeys, shards)
            table.ops[(clock, dot)] = p
            ex.live.setdefault(dot, []).append(p)
            ex.nlive += 1
            ex.max_live = max(ex.max_live, ex.nlive)
        try:
            table.add_votes(votes)
        except VoteError:
            if kind == "A":  # the event leaves no trace
                del table.ops[(clock, dot)]
                ex.live[dot].remove(p)
                ex.nlive -= 1
            return FX_ERR_VOTE_RANGE
        try:
            ex.send_stable_or_execute(key, table.stable_ops())
            ex.max_stack = max(ex.max_stack, len(ex.to_executors))
            ex.drain()
        except CountError:
            return FX_ERR_INVALID_ARG
        return FX_OK

    def result(self):
        """What table_ref_mk.run_stream returns, and: sent (event row -> the
        step during which that partial made its command stable at the shard),
        max_buffered_pairs (the most (key, rifl) pairs buffered at once) and
        max_count (the highest buffered count)."""
        ex = self.ex
        stable = [ex.tables[k].stable_clock() if k in ex.tables else 0 for k in range(self.keys)]
        return dict(order=list(ex.order), release=dict(ex.release), nexec=len(ex.order), err=self.err, stable=stable,
                    max_live=ex.max_live, max_stack=ex.max_stack, buffered=ex.buffered_msgs,
                    unhandled=len(ex.to_executors), max_above=max([t.max_above for t in ex.tables.values()] + [0]),
                    max_gap_above=max([t.max_gap_above for t in ex.tables.values()] + [0]),
                    sent=dict(ex.sent), max_buffered_pairs=ex.max_buffered_pairs, max_count=ex.max_count)


def run_stream(events, n, stability_threshold, keys, vmax=None, execute_at_commit=False):
    """One executor's stream: Stream.result() after its events."""
    st = Stream(n, stability_threshold, keys, vmax, execute_at_commit)
    for ev in events:
        if st.feed(ev) != FX_OK:
            break
    return st.result()
