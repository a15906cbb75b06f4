"""Shared inputs of the multi-key table-executor tests: hand-written streams
with the order and release written out from the reference's
fantoch_ps/src/executor/table/executor.rs, the generated multi-key streams,
and the restatement's results (tests/table_ref_mk.py) computed once per case."""
import functools

from fantoch_amd import table as ft

import table_ref_mk as RM
from table_shapes import quorum_sizes

# n = 3, f = 1: stability threshold 2, so an op is stable on its key once two
# of the three processes voted up to its clock
HAND_N, HAND_THR, HAND_KEYS = 3, 2, 3
X, Y, Z, S1 = (1, 1), (2, 1), (3, 1), (2, 7)


def att(key, dot, clock, lo, nkeys):
    """An attached event that makes its op stable on `key` at once: processes
    1 and 2 vote lo..clock."""
    return ("A", key, dot, clock, [(1, lo, clock), (2, lo, clock)], nkeys)


# name -> (events, order, release, unhandled); order holds event rows
HAND = {
    # X is stable on key 0 at event 0 and waits there for its other key
    # (:319-328, count 1 of 2).  Event 2 makes it stable on key 1: the count
    # reaches 2, StableAtShard(key 0) is pushed and X executes on key 1
    # (:328-352); the same event's drain hands the message to key 0 (:173-195).
    "late_key": ([att(0, X, 1, 1, 2), att(2, S1, 1, 1, 1), att(1, X, 1, 1, 2)],
                 [1, 2, 0], {1: 1, 2: 2, 0: 2}, 0),
    # the single-key S1 becomes stable on key 0 behind the waiting X: the queue
    # is not empty, so it joins it untried (:242-247) and executes only after
    # X, in the drain of event 2 (:198-217)
    "behind_head": ([att(0, X, 1, 1, 2), att(0, S1, 2, 2, 1), att(1, X, 1, 1, 2)],
                    [2, 0, 1], {2: 2, 0: 2, 1: 2}, 0),
    "behind_head_prefix": ([att(0, X, 1, 1, 2), att(0, S1, 2, 2, 1)], [], {}, 0),
    # Y (keys 0 and 2) waits on key 2 and sits behind X on key 0.  Event 3
    # completes X; its drain executes X on key 0 and then tries Y there, whose
    # last key this is: Y executes on key 0 and StableAtShard(key 2, Y) is
    # pushed during the drain, so it is handled by the drain of event 4
    "chain": ([att(0, X, 1, 1, 2), att(2, Y, 2, 1, 2), att(0, Y, 2, 2, 2), att(1, X, 1, 1, 2),
               ("D", 1, [(3, 1, 1)])],
              [3, 0, 2, 1], {3: 3, 0: 3, 2: 3, 1: 4}, 0),
    # the same without event 4: the message is never handled (runner.rs:411-416)
    "chain_cut": ([att(0, X, 1, 1, 2), att(2, Y, 2, 1, 2), att(0, Y, 2, 2, 2), att(1, X, 1, 1, 2)],
                  [3, 0, 2], {3: 3, 0: 3, 2: 3}, 1),
    # three keys: the messages go to keys 0 and 2 in that order (C13) and come
    # back last first, so key 2 (event 1) executes before key 0 (event 0)
    "three_keys": ([att(0, Z, 1, 1, 3), att(2, Z, 1, 1, 3), att(1, Z, 1, 1, 3)],
                   [2, 1, 0], {2: 2, 1: 2, 0: 2}, 0),
}

# generated streams: (n, f, tiny quorums), most keys per command, conflict rates
CONFIGS = [(3, 1, False), (5, 1, False)]
KMAX = [2, 3]
CONFLICTS = [0, 10, 50, 100]
SEEDS, KEYS, CMDS, LAG, WINDOW = 24, 16, 120, 2, 2


@functools.lru_cache(maxsize=None)
def generated(n, f, tiny, kmax, conflict, count=SEEDS, cmds=CMDS, lag=LAG, window=WINDOW, keys=KEYS):
    fq = quorum_sizes(n, f, tiny)[0]
    return tuple(tuple(ft.synth_table_streams_mk(100000 * kmax + 1000 * conflict + seed, n, fq, keys, cmds, conflict,
                                                 lag, window, kmax)) for seed in range(count))


@functools.lru_cache(maxsize=None)
def generated_ref(n, f, tiny, kmax, conflict, count=SEEDS, cmds=CMDS, lag=LAG, window=WINDOW, keys=KEYS):
    thr = quorum_sizes(n, f, tiny)[2]
    return tuple(RM.run_stream(list(st), n, thr, keys)
                 for st in generated(n, f, tiny, kmax, conflict, count, cmds, lag, window, keys))
