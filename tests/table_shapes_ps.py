"""Shared inputs of the tests of the table executor over several shards:
hand-written streams with the order, release and stable_sent rows written out
from the reference's fantoch_ps/src/executor/table/executor.rs, the generator
of groups of shard executors co-simulated with the restatement
(tests/table_ref_ps.py), and the restatement's results computed once per case."""
import functools
import random

import table_ref_ps as RP
from table_ref import FX_ERR_INVALID_ARG
from table_shapes import quorum_sizes

# n = 3, f = 1: stability threshold 2, so an op is stable on its key once two
# of the three processes voted up to its clock
HAND_N, HAND_THR, HAND_KEYS = 3, 2, 3
X, Y, Z, S1, S2, S3 = (1, 1), (2, 1), (3, 1), (2, 7), (3, 2), (3, 3)


def att(key, dot, clock, lo, nkeys, shards):
    """An attached event that makes its op stable on `key` at once: processes
    1 and 2 vote lo..clock."""
    return ("A", key, dot, clock, [(1, lo, clock), (2, lo, clock)], nkeys, shards)


def st(key, dot):
    return ("S", key, dot)


# name -> (events, order, release, sent, err); order holds event rows
HAND = {
    # 1. two shards, one key here: X is stable here at event 0, tells the other
    # shard at once (:311-316, sent at its own step) and waits with one shard
    # missing (:353-357); the other shard's message executes it (:173-195)
    "wait_then_msg": ([att(0, X, 1, 1, 1, 2), st(0, X)], [0], {0: 1}, {0: 0}, 0),
    # 2. the message first: the queue is empty, so it is buffered (:227-234) and
    # counted when X is tried (:345-347): 2 - 1 (own shard) - 1 = 0
    "msg_then_stable": ([st(0, X), att(0, X, 1, 1, 1, 2)], [1], {1: 1}, {1: 1}, 0),
    # 3. three shards: both messages buffered (count 2) ...
    "three_both_buffered": ([st(0, X), st(0, X), att(0, X, 1, 1, 1, 3)], [2], {2: 2}, {2: 2}, 0),
    # ... and one buffered, one to the waiting head
    "three_one_each": ([st(0, X), att(0, X, 1, 1, 1, 3), st(0, X)], [1], {1: 2}, {1: 1}, 0),
    # 4. two keys here, two shards; the other shard's messages before local
    # stability: each key has one buffered.  Key 0 tries first (count 1 of 2,
    # 2 - 1 = 1 missing); key 1's try makes the count 2: it is the sender, tells
    # key 0 through to_executors and executes (2 - 1 - 1); the drain of the same
    # event brings key 0 its message: the local message still travels
    "two_keys_msgs_first": ([st(0, X), st(1, X), att(0, X, 1, 1, 2, 2), att(1, X, 1, 1, 2, 2)],
                            [3, 2], {3: 3, 2: 3}, {3: 3}, 0),
    # the other shard's messages after local stability: at event 1 key 1 is the
    # sender (1 missing) and the drain takes key 0 from 2 to 1; then the remote
    # messages execute key 1 and key 0
    "two_keys_msgs_last": ([att(0, X, 1, 1, 2, 2), att(1, X, 1, 1, 2, 2), st(1, X), st(0, X)],
                           [1, 0], {1: 2, 0: 3}, {1: 1}, 0),
    # 5. X waits for the other shard at the head of key 0; two single-key ops, a
    # two-shard op Z and another single-key op queue up behind it (:242-247).
    # The message executes X and then the queue in FIFO order (:198-217) until
    # Z, which is tried (sent at step 5) and handed back; the last op stays
    "followers": ([att(0, X, 1, 1, 1, 2), att(0, S1, 2, 2, 1, 1), att(0, S2, 3, 3, 1, 1), att(0, Z, 4, 4, 1, 2),
                   att(0, S3, 5, 5, 1, 1), st(0, X)],
                  [0, 1, 2], {0: 5, 1: 5, 2: 5}, {0: 0, 3: 5}, 0),
    # 6. the message for Y, queued behind X, is buffered (:219-226: the head is
    # another command) and counted when Y is tried after X executed
    "msg_for_queued": ([att(0, X, 1, 1, 1, 2), att(0, Y, 2, 2, 1, 2), st(0, Y), st(0, X)],
                       [0, 1], {0: 3, 1: 3}, {0: 0, 1: 3}, 0),
    # 7. a message for a rifl that never arrives stays buffered: no error
    "msg_for_nobody": ([att(0, S1, 1, 1, 1, 1), st(1, X)], [0], {0: 0}, {}, 0),
    # 8. two messages buffered for a two-shard command: the count is above what
    # is missing after the own shard (1): the stream stops, event 0's rows stay
    "count_above_missing": ([att(1, S1, 1, 1, 1, 1), st(0, X), st(0, X), att(0, X, 1, 1, 1, 2)],
                            [0], {0: 0}, {}, FX_ERR_INVALID_ARG),
    # 9. another `shards` for the dot, shards 0, shards 9
    "shards_differ": ([att(2, S1, 1, 1, 1, 1), att(0, X, 1, 1, 2, 2), att(1, X, 1, 1, 2, 3)],
                      [0], {0: 0}, {}, FX_ERR_INVALID_ARG),
    "shards_zero": ([att(2, S1, 1, 1, 1, 1), att(0, X, 1, 1, 1, 0)], [0], {0: 0}, {}, FX_ERR_INVALID_ARG),
    "shards_nine": ([att(2, S1, 1, 1, 1, 1), att(0, X, 1, 1, 1, 9)], [0], {0: 0}, {}, FX_ERR_INVALID_ARG),
}


def synth_table_group(seed, shards, n, fast_quorum, stability_threshold, keys, cmds, conflict_pct, lag, window, kmax,
                      smax, msg_lag):
    """A group of `shards` shard executors over `cmds` commands, each stream
    co-simulated with the restatement.  Returns (streams, commands, results):
    one event stream per shard, the map dot -> {shard: [keys]}, and each
    shard's restatement result.

    A command picks 1..smax shards (uniform) and 1..kmax keys on each; on a
    shard its first key is key 0 with probability conflict_pct percent.  Every
    shard has its own n processes with a clock per key; on each shard the
    coordinator's and the fast quorum's proposals and votes are what
    fantoch_amd.table.synth_table_streams_mk produces over the command's keys
    there, the commit clock is the highest proposal over all the command's
    keys on all its shards (fantoch_ps/src/protocol/tempo.rs:614-636), and
    every process below it votes up to it as a detached range.  A shard's own
    events are delivered as in synth_table_streams_mk (`window`, `lag`).

    Rounds: in round t every shard first handles the StableAtShard messages
    due, then its own event t.  When a shard's restatement reports `sent` for
    a command in round t, each key of the command on another shard gets a
    message due at round t + 1 + rng(msg_lag), ascending by (shard, key);
    messages due after a shard's last own event are appended to its stream."""
    rng = random.Random(seed)
    G = shards
    clocks = [[[0] * keys for _ in range(n + 1)] for _ in range(G)]
    seqs = [0] * (n + 1)
    own = [[] for _ in range(G)]  # (delivery slot, creation index, event)
    commands = {}
    for i in range(cmds):
        on = sorted(rng.sample(range(G), 1 + rng.randrange(min(smax, G))))
        p = 1 + rng.randrange(n)
        seqs[p] += 1
        dot = (p, seqs[p])
        cmd, votes, commit = {}, {}, 0
        for g in on:
            k = 1 + rng.randrange(min(kmax, keys))
            first = 0 if keys == 1 or rng.randrange(100) < conflict_pct else 1 + rng.randrange(keys - 1)
            cmd[g] = sorted([first] + rng.sample([x for x in range(keys) if x != first], k - 1))
            others = rng.sample([q for q in range(1, n + 1) if q != p], fast_quorum - 1)
            ck = clocks[g]
            prop = max(ck[p][x] for x in cmd[g]) + 1
            for x in cmd[g]:
                votes[g, x] = [(p, ck[p][x] + 1, prop)]
                ck[p][x] = prop
            commit = max(commit, prop)
            for q in others:
                pq = max(prop, max(ck[q][x] for x in cmd[g]) + 1)
                for x in cmd[g]:
                    votes[g, x].append((q, ck[q][x] + 1, pq))
                    ck[q][x] = pq
                commit = max(commit, pq)
        commands[dot] = cmd
        for g in on:
            slot = i + rng.randrange(window + 1)
            for x in cmd[g]:
                own[g].append((slot, len(own[g]), ("A", x, dot, commit, votes[g, x], len(cmd[g]), len(on))))
            for x in cmd[g]:
                for q in range(1, n + 1):
                    if clocks[g][q][x] < commit:
                        vr = (q, clocks[g][q][x] + 1, commit)
                        clocks[g][q][x] = commit
                        own[g].append((i + rng.randrange(lag + 1), len(own[g]), ("D", x, [vr])))
    own = [[e[2] for e in sorted(o, key=lambda e: (e[0], e[1]))] for o in own]

    sims = [RP.Stream(n, stability_threshold, keys) for _ in range(G)]
    streams = [[] for _ in range(G)]
    due = [[] for _ in range(G)]  # (round, send index, key, dot)
    nsent, t = 0, 0

    def feed(g, ev):
        nonlocal nsent
        before = set(sims[g].ex.sent)
        assert sims[g].feed(ev) == 0
        streams[g].append(ev)
        for a in sorted(set(sims[g].ex.sent) - before):
            dot = streams[g][a][2]
            for h in sorted(commands[dot]):
                if h != g:
                    for x in commands[dot][h]:
                        due[h].append((t + 1 + rng.randrange(msg_lag + 1), nsent, x, dot))
                        nsent += 1

    while any(t < len(own[g]) or due[g] for g in range(G)):
        for g in range(G):
            now = sorted(m for m in due[g] if m[0] <= t)
            due[g] = [m for m in due[g] if m[0] > t]
            for _, _, x, dot in now:
                feed(g, ("S", x, dot))
            if t < len(own[g]):
                feed(g, own[g][t])
        t += 1
    return streams, commands, [s.result() for s in sims]


# generated groups: (shards, n, f), conflict rates; 60 commands per shard
# executor on average; lag, window and msg_lag were chosen on the CPU
# (tests/test_table_ps_ref.py::test_generated_groups_cover_the_branches)
GROUPS = [(2, 5, 1), (3, 5, 1), (2, 3, 1), (3, 3, 1)]
CONFLICTS = [10, 100]
SEEDS, KEYS, KMAX, PER_SHARD, LAG, WINDOW, MSG_LAG = 8, 16, 2, 60, 4, 0, 3


def group_cmds(shards, per_shard=PER_SHARD):
    """Commands of a group so that a shard sees about per_shard of them: a
    command picks 1..shards shards, (shards + 1) / 2 on average."""
    return per_shard * shards * 2 // (shards + 1)


@functools.lru_cache(maxsize=None)
def generated(shards, n, f, conflict, count=SEEDS, per_shard=PER_SHARD, lag=LAG, window=WINDOW, msg_lag=MSG_LAG,
              keys=KEYS, kmax=KMAX):
    """`count` groups (seeds 0..count-1) of one configuration: a tuple of
    (streams, commands, results)."""
    fq, _, thr = quorum_sizes(n, f, False)
    return tuple(synth_table_group(70000 * shards + 1000 * conflict + 10 * n + seed, shards, n, fq, thr, keys,
                                   group_cmds(shards, per_shard), conflict, lag, window, kmax, shards, msg_lag)
                 for seed in range(count))


def s_events(streams):
    """The StableAtShard events of a group's streams as (shard, key, dot), sorted."""
    return sorted((g, ev[1], ev[2]) for g, stream in enumerate(streams) for ev in stream if ev[0] == "S")


def fits_onchip(ref):
    """The restatement says the stream stays inside the ONCHIP tier of fx_table_execute_ps."""
    from fantoch_amd import _lib
    return (ref["max_live"] <= _lib.FX_TABLE_MK_ONCHIP_LIVE and ref["max_stack"] <= _lib.FX_TABLE_MK_ONCHIP_STACK
            and ref["max_gap_above"] <= _lib.FX_TABLE_ONCHIP_WINDOW
            and ref["max_buffered_pairs"] <= _lib.FX_TABLE_PS_ONCHIP_BUFFERED)


def fits_hbm(ref):
    from fantoch_amd import _lib
    return (ref["max_live"] <= _lib.FX_TABLE_MK_HBM_LIVE and ref["max_stack"] <= _lib.FX_TABLE_MK_HBM_STACK
            and ref["max_above"] <= _lib.FX_TABLE_HBM_WINDOW
            and ref["max_buffered_pairs"] <= _lib.FX_TABLE_PS_HBM_BUFFERED)
