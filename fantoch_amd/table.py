"""Host side of the batched Tempo TableExecutor (fx_table_*): packing streams
of TableExecutionInfo values into planes, Tempo's quorum sizes, and a
deterministic Tempo-shaped stream generator.

An event is ("A", key, (source, seq), clock, votes[, nkeys]) -- AttachedVotes
-- or ("D", key, votes) -- DetachedVotes -- with votes a list of
(voter, start, end) ranges (fantoch_ps/src/executor/table/executor.rs:110-144)
and key a dense id below `keys`.  nkeys (1 when absent) is the number of keys
of the event's command: Tempo emits one AttachedVotes per key, each with the
command's dot and clock (fantoch_ps/src/protocol/tempo.rs:614-636).

Commands that span shards (fx_table_*_ps): an attached event may carry a
seventh element, shards -- the number of shards its command accesses, this
one included (1 when absent); nkeys then counts the command's keys at this
shard -- and ("S", key, (source, seq)) is a StableAtShard{key, rifl} that
another shard's executor sent (executor.rs:140-142; the rifl is the dot).

Seeded streams on the canonical counter RNG (fx_table_synth_*): the library
generates them on the device (fantoch_amd.device.synth_table) or on the host
(synth_table_host, the same bytes), and synth_table_streams_c6 restates the
model in plain Python.  The same for the closed-loop shard groups of
fx_table_run_groups (fx_table_group_synth_*): fantoch_amd.device
.synth_table_groups, synth_table_groups_host and synth_table_groups_c6.
"""
import ctypes
import random

import numpy as np

from . import _lib
from ._lib import index, pack_dot, plane_words


def table_hdr(kind, nvotes, key):
    """FX_TABLE_HDR."""
    return ((int(kind) & 1) << 31) | ((int(nvotes) & 127) << 24) | (int(key) & 0xFFFFFF)


STABLE_NVOTES = 127  # the vote-count field of a StableAtShard event's header


def table_hdr_stable(key):
    """FX_TABLE_HDR_STABLE."""
    return table_hdr(_lib.FX_TABLE_DETACHED, STABLE_NVOTES, key)


def table_ps_word(nkeys, shards):
    """FX_TABLE_PS_WORD."""
    return (int(nkeys) | (int(shards) << 8)) & 0xFFFFFFFF


class TablePlanes:
    """Host copy of an fx_table_batch: hdr / dot / clock planes, 3 * vmax vote
    planes, lengths; nkeys is None or the extra plane of an fx_table_batch_mk.
    ps: the batch holds StableAtShard events or commands that span shards, and
    the nkeys plane (if any) holds FX_TABLE_PS_WORD(nkeys, shards) words."""

    def __init__(self, num_streams, steps, n, keys, vmax, lengths=None):
        self.S, self.steps, self.n, self.keys, self.vmax = int(num_streams), int(steps), int(n), int(keys), int(vmax)
        self.plane = plane_words(self.S, self.steps)
        self.hdr = np.zeros(self.plane, np.uint32)
        self.dot = np.zeros(self.plane, np.uint32)
        self.clock = np.zeros(self.plane, np.uint32)
        self.votes = np.zeros(3 * self.vmax * self.plane, np.uint32)
        self.lengths = lengths
        self.nkeys = None
        self.ps = False

    def stream(self, s, start=0):
        """Decodes stream s (from row `start` on) back into its list of events."""
        L = self.steps if self.lengths is None else int(self.lengths[s])
        out = []
        for at in index(np.arange(start, L), s, self.steps):
            at = int(at)
            h = int(self.hdr[at])
            key, nv = h & 0xFFFFFF, (h >> 24) & 127
            if self.ps and h >> 31 == _lib.FX_TABLE_DETACHED and nv == STABLE_NVOTES:
                out.append(("S", key, _lib.unpack_dot(self.dot[at])))
                continue
            votes = [tuple(int(self.votes[(3 * j + c) * self.plane + at]) for c in range(3)) for j in range(nv)]
            if h >> 31 == _lib.FX_TABLE_ATTACHED:
                ev = ("A", key, _lib.unpack_dot(self.dot[at]), int(self.clock[at]), votes)
                w = 1 if self.nkeys is None else int(self.nkeys[at])
                if self.ps and w >> 8 != 1:
                    ev += (w & 0xFF, w >> 8)
                elif (w & 0xFF if self.ps else w) != 1:
                    ev += (w & 0xFF if self.ps else w,)
                out.append(ev)
            else:
                out.append(("D", key, votes))
        return out


def _votes(ev):
    return ev[4] if ev[0] == "A" else ev[2] if ev[0] == "D" else ()


def pack_table_streams(streams, n, keys):
    """streams: lists of ("A", key, (src, seq), clock, votes[, nkeys[, shards]])
    / ("D", key, votes) / ("S", key, (src, seq)) events.  The nkeys plane is
    filled when an event has nkeys other than 1 (fantoch_amd.device.run_table
    then takes the _mk entry points).  With an "S" event or a `shards` other
    than 1 anywhere the planes are marked `ps`, the nkeys plane holds
    FX_TABLE_PS_WORD(nkeys, shards) and run_table takes the _ps entry points;
    streams without either pack exactly as before.  Raises ValueError on what
    the planes cannot hold: a key outside 0..keys-1, a clock or vote at or
    above 2**32, more than FX_TABLE_MAX_VOTES ranges in an event, nkeys outside
    32 bits (in `ps` planes: 8 bits, or above `keys`), shards outside 24 bits."""
    S = len(streams)
    steps = max([len(s) for s in streams] + [1])
    vmax = max([len(_votes(ev)) for st in streams for ev in st] + [1])
    if vmax > _lib.FX_TABLE_MAX_VOTES:
        raise ValueError("an event carries %d vote ranges (at most %d)" % (vmax, _lib.FX_TABLE_MAX_VOTES))
    if not 1 <= keys <= _lib.FX_TABLE_MAX_KEYS:
        raise ValueError("keys = %d" % keys)
    p = TablePlanes(S, steps, n, keys, vmax, lengths=np.array([len(s) for s in streams], np.uint32))
    p.ps = any(ev[0] == "S" or (ev[0] == "A" and len(ev) == 7 and int(ev[6]) != 1) for st in streams for ev in st)
    for s, st in enumerate(streams):
        if not st:
            continue
        idx = index(np.arange(len(st)), s, steps)
        for i, ev in enumerate(st):
            _pack_event(p, int(idx[i]), ev)
    return p


def _pack_event(p, at, ev):
    """Writes one event into the planes p at plane position `at`."""
    keys = p.keys
    kind, key = ev[0], int(ev[1])
    if kind not in ("A", "D", "S") or len(ev) not in ((5, 6, 7) if kind == "A" else (3,)):
        raise ValueError("malformed event %r" % (ev,))
    votes = _votes(ev)
    if not 0 <= key < keys:
        raise ValueError("key %d outside 0..%d" % (key, keys - 1))
    if kind != "D":
        src, seq = ev[2]
        if not (0 <= int(src) < 256 and 0 <= int(seq) <= _lib.FX_SEQ_MASK):
            raise ValueError("dot %r does not fit the packed form" % ((src, seq),))
        p.dot[at] = pack_dot(src, seq)
    if kind == "S":
        p.hdr[at] = table_hdr_stable(key)
        return
    if kind == "A":
        clock = int(ev[3])
        if not 0 <= clock < 1 << 32:
            raise ValueError("clock %d does not fit 32 bits" % clock)
        p.clock[at] = clock
        nk = int(ev[5]) if len(ev) >= 6 else 1
        sh = int(ev[6]) if len(ev) == 7 else 1
        if not 0 <= nk < (1 << 8 if p.ps else 1 << 32):
            raise ValueError("nkeys %d does not fit %d bits" % (nk, 8 if p.ps else 32))
        if not 0 <= sh < 1 << 24:
            raise ValueError("shards %d does not fit 24 bits" % sh)
        if p.ps and nk > keys:  # (the keys of a command at a shard are distinct keys of that shard)
            raise ValueError("nkeys %d with %d keys at the shard" % (nk, keys))
        word = table_ps_word(nk, sh) if p.ps else nk
        if word != (table_ps_word(1, 1) if p.ps else 1) and p.nkeys is None:
            p.nkeys = np.full(p.plane, table_ps_word(1, 1) if p.ps else 1, np.uint32)
        if p.nkeys is not None:
            p.nkeys[at] = word
    p.hdr[at] = table_hdr(_lib.FX_TABLE_ATTACHED if kind == "A" else _lib.FX_TABLE_DETACHED, len(votes), key)
    for j, vr in enumerate(votes):
        for c in range(3):
            if not 0 <= int(vr[c]) < 1 << 32:
                raise ValueError("vote range %r does not fit 32 bits" % (vr,))
            p.votes[(3 * j + c) * p.plane + at] = int(vr[c])


def sent_rows(planes, stable_sent, s):
    """The (dot, step) pairs of stream s whose stable_sent row is set: the
    commands the shard's executor reported stable at the shard and when, in
    ascending (step, event row) order.  stable_sent: the plane
    fantoch_amd.device.run_table returns."""
    L = planes.steps if planes.lengths is None else int(planes.lengths[s])
    at = index(np.arange(L), s, planes.steps)
    rows = [(int(stable_sent[a]), r, _lib.unpack_dot(planes.dot[a])) for r, a in enumerate(at)
            if stable_sent[a] != _lib.FX_RELEASE_NONE]
    return [(dot, step) for step, _, dot in sorted(rows)]


def stable_messages(sent, commands, shard):
    """The StableAtShard messages a host routes for one shard's result.
    sent: that shard's (dot, step) pairs (sent_rows); commands: the group's
    map dot -> {shard: [keys]} (the command's shard_to_keys); shard: the shard
    the result belongs to.  Returns (target shard, key, dot, step) tuples: per
    pair, one for every key of the command at every other shard, ascending by
    (shard, key) -- DESIGN.md C13 extended to shards; the keys at `shard`
    itself were told through the executor's own to_executors."""
    out = []
    for dot, step in sent:
        for target in sorted(commands[dot]):
            if target != shard:
                out.extend((target, key, dot, step) for key in sorted(commands[dot][target]))
    return out


def run_table_groups(groups, n, keys, stability_threshold, delay=None, execute_at_commit=False, session=None):
    """Groups of shard executors run in a closed loop: the StableAtShard
    messages an executor sends reach the other executors of its group as
    ("S", key, dot) events of their streams, routed here from stable_sent.

    groups: a list of (own, commands); own[g] is shard g's own events ("A" /
    "D") in order, commands the group's map dot -> {shard: [keys]} (as
    stable_messages takes it).  All streams of all groups advance together,
    one fx_table_advance per round (fantoch_amd.device.TableSession,
    FX_TABLE_KIND_PS).  Delivery: in round t every shard first
    handles the messages due, ascending by (due round, send index), then its
    own event t.  A message sent in round t is due at round
    t + 1 + delay(sender, dot, target, key) (delay None: 0).  A group's send
    indices count up over its rounds, within a round over its shards
    ascending, per shard by (stable_sent step, event row), then over target
    shard and key ascending.  Messages due after a shard's last own event are
    appended; the loop ends when no own events and no messages are left.  A
    shard whose stream stops with an error handles nothing more and messages
    to it are dropped; the other shards go on.

    session: a factory taking TableSession's arguments for the object whose
    advance(planes) runs the executors (default: TableSession).
    Returns one dict per group: streams (per shard the events as handled,
    the "S" events in place), results (per shard order -- event rows --,
    release and sent -- event row -> step --, nexec, err, stable, all relative
    to those rows) and rounds."""
    if session is None:
        from . import device
        session = device.TableSession
    where, first = [], []
    for i, (own, _) in enumerate(groups):
        first.append(len(where))
        where.extend((i, g) for g in range(len(own)))
    S = len(where)
    steps = group_steps_out(groups)
    vmax = max([len(_votes(ev)) for own, _ in groups for st in own for ev in st] + [1])
    p = TablePlanes(S, steps, n, keys, vmax, lengths=np.zeros(S, np.uint32))
    p.ps = True
    p.nkeys = np.full(p.plane, table_ps_word(1, 1), np.uint32)
    sess = session(S, steps, n, keys, vmax, stability_threshold, _lib.FX_TABLE_KIND_PS, execute_at_commit)
    streams = [[] for _ in range(S)]
    due = [[] for _ in range(S)]  # (due round, send index, key, dot)
    seen = np.zeros((S, steps), bool)  # rows whose stable_sent was routed
    stopped = [False] * S
    nsent, rounds = [0] * len(groups), [0] * len(groups)
    res, t = None, 0

    def left(s):
        return not stopped[s] and (t < len(groups[where[s][0]][0][where[s][1]]) or bool(due[s]))

    while any(left(s) for s in range(S)):
        for s, (i, g) in enumerate(where):
            if not left(s):
                continue
            rounds[i] = t + 1
            own = groups[i][0][g]
            now = sorted(m for m in due[s] if m[0] <= t)
            due[s] = [m for m in due[s] if m[0] > t]
            for ev in [("S", x, dot) for _, _, x, dot in now] + ([own[t]] if t < len(own) else []):
                _pack_event(p, int(index(len(streams[s]), s, steps)), ev)
                streams[s].append(ev)
            p.lengths[s] = len(streams[s])
        res = sess.advance(p)
        for s, (i, g) in enumerate(where):
            if stopped[s]:
                continue
            sent = res.stable_sent[index(np.arange(len(streams[s])), s, steps)]
            new = np.nonzero((sent != _lib.FX_RELEASE_NONE) & ~seen[s, :len(sent)])[0]
            commands = groups[i][1]
            for _, a in sorted((int(sent[a]), int(a)) for a in new):
                seen[s, a] = True
                dot = streams[s][a][2]
                for target, x, _, _ in stable_messages([(dot, 0)], commands, g):
                    lag = int(delay(g, dot, target, x)) if delay is not None else 0
                    due[first[i] + target].append((t + 1 + lag, nsent[i], x, dot))
                    nsent[i] += 1
            if res.err[s]:
                stopped[s] = True
        for s in range(S):
            if stopped[s]:
                due[s] = []
        t += 1

    out = []
    for i, (own, _) in enumerate(groups):
        results = []
        for s in range(first[i], first[i] + len(own)):
            if res is None:
                results.append(dict(order=[], release={}, sent={}, nexec=0, err=0, stable=[0] * keys))
                continue
            rows = index(np.arange(len(streams[s])), s, steps)
            planes = {name: {a: int(v) for a, v in enumerate(pl[rows]) if v != _lib.FX_RELEASE_NONE}
                      for name, pl in (("release", res.release), ("sent", res.stable_sent))}
            nexec = int(res.nexec[s])
            order = [int(x) & ~_lib.FX_ORDER_SCC_START for x in res.order[index(np.arange(nexec), s, steps)]]
            results.append(dict(order=order, release=planes["release"], sent=planes["sent"], nexec=nexec,
                                err=int(res.err[s]), stable=[int(x) for x in res.stable_clock[s]]))
        out.append(dict(streams=streams[first[i]:first[i] + len(own)], results=results, rounds=rounds[i]))
    return out


def table_target(delay, shard, key):
    """FX_TABLE_TARGET."""
    return ((int(delay) << 27) | ((int(shard) & 7) << 24) | (int(key) & 0xFFFFFF)) & 0xFFFFFFFF


def _stream_rows(own, commands, g):
    """Rows shard g's stream can come to: its own events plus one per (key
    here, other shard) of every command that spans shards."""
    return len(own[g]) + sum(len(cmd[g]) * (len(cmd) - 1) for cmd in commands.values() if g in cmd)


def group_steps_out(groups):
    """Rows a group stream can come to (the plane rows of run_table_groups):
    the highest over all streams, at least 1."""
    return max([_stream_rows(own, commands, g) for own, commands in groups for g in range(len(own))] + [1])


def pack_table_groups(groups, n, keys, delay=None):
    """The input of fx_table_run_groups (fantoch_amd.device.run_table_groups)
    for groups as run_table_groups takes them: a list of (own, commands), all
    with the same number of shards.  Returns (planes, route, targets,
    steps_out): the TablePlanes of the own events (stream g * shards + h =
    shard h of group g), the route plane over their rows, the targets array
    and the rows of the output planes (group_steps_out).  The attached events
    of a command that spans shards point at the command's list in targets:
    its length m, then one FX_TABLE_TARGET(delay, shard, key) per key of the
    command at every other shard, ascending by (shard, key) as stable_messages
    gives them; the events of one command at one shard share one list.
    delay(sender, dot, target, key) is evaluated here and must lie in
    0..FX_TABLE_GROUP_MAX_DELAY (None: 0).  Raises ValueError on that, on
    groups of different shard counts, and on what pack_table_streams refuses."""
    counts = {len(own) for own, _ in groups}
    if len(counts) > 1:
        raise ValueError("groups of %s shards in one call" % sorted(counts))
    P = counts.pop() if counts else 1
    if not 1 <= P <= _lib.FX_TABLE_MAX_CMD_SHARDS:
        raise ValueError("%d shards in a group (1..%d)" % (P, _lib.FX_TABLE_MAX_CMD_SHARDS))
    p = pack_table_streams([st for own, _ in groups for st in own], n, keys)
    if p.nkeys is None:
        p.nkeys = np.full(p.plane, 1 if not p.ps else table_ps_word(1, 1), np.uint32)
    if not p.ps:  # plain nkeys words: one shard each (a word that is no nkeys stays invalid)
        p.nkeys = np.where(p.nkeys < 256, p.nkeys | np.uint32(1 << 8), np.uint32(0)).astype(np.uint32)
        p.ps = True
    route = np.full(p.plane, _lib.FX_TABLE_ROUTE_NONE, np.uint32)
    targets = []
    for i, (own, commands) in enumerate(groups):
        lists = {}  # (shard, dot) -> index into targets
        for h, st in enumerate(own):
            s = i * P + h
            for r, ev in enumerate(st):
                if ev[0] != "A" or len(ev) != 7 or int(ev[6]) <= 1:
                    continue
                dot = ev[2]
                if dot not in commands or h not in commands[dot]:
                    raise ValueError("group %d: command %r is not at shard %d" % (i, dot, h))
                if (h, dot) not in lists:
                    lists[h, dot] = len(targets)
                    msgs = stable_messages([(dot, 0)], commands, h)
                    targets.append(len(msgs))
                    for target, key, _, _ in msgs:
                        lag = int(delay(h, dot, target, key)) if delay is not None else 0
                        if not 0 <= lag <= _lib.FX_TABLE_GROUP_MAX_DELAY:
                            raise ValueError("delay %d outside 0..%d" % (lag, _lib.FX_TABLE_GROUP_MAX_DELAY))
                        if not (0 <= target < P and 0 <= key < keys):
                            raise ValueError("command %r: key %d at shard %d" % (dot, key, target))
                        targets.append(table_target(lag, target, key))
                route[int(index(r, s, p.steps))] = lists[h, dot]
    return p, route, np.array(targets, np.uint32), group_steps_out(groups)


def handled_stream(own, src, dot):
    """A group stream as handled, rebuilt from its rows of the handled_src and
    handled_dot planes of fx_table_run_groups: row j is the own event
    own[src[j]], or for FX_TABLE_HANDLED_MSG | key the routed ("S", key, dot)."""
    out = []
    for x, d in zip(src, dot):
        x = int(x)
        out.append(("S", x & 0xFFFFFF, _lib.unpack_dot(d)) if x & _lib.FX_TABLE_HANDLED_MSG else own[x])
    return out


def tempo_quorum_sizes(n, f, tiny_quorums=False):
    """(fast quorum, write quorum, stability threshold): Config::tempo_quorum_sizes
    (fantoch/src/config.rs:337-349) via fx_tempo_quorum_sizes."""
    fq, wq, st = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    _lib.check(_lib.load().fx_tempo_quorum_sizes(n, f, 1 if tiny_quorums else 0, ctypes.byref(fq), ctypes.byref(wq),
                                                 ctypes.byref(st)), "fx_tempo_quorum_sizes")
    return fq.value, wq.value, st.value


def synth_table_streams(seed, n, fast_quorum, keys, cmds, conflict_pct, lag, window):
    """One deterministic Tempo-shaped stream of `cmds` single-key commands.

    Every process keeps a clock per key (SequentialKeyClocks,
    protocol/common/table/clocks/keys/sequential.rs:38-114).  A command goes to
    key 0 with probability conflict_pct percent and otherwise to a uniform
    other key; a random coordinator p and fast_quorum - 1 other processes form
    its fast quorum.  p proposes own + 1, every other member
    max(p's proposal, own + 1); each votes the range own + 1 .. its proposal
    (proposal, sequential.rs:38-57) and the commit clock is the highest
    proposal.  Then every process whose clock for the key is below the commit
    clock votes own + 1 .. commit clock as a detached range (detached,
    sequential.rs:59-70, 99-114), delivered up to `lag` commands later; the
    commit itself (AttachedVotes with the quorum's ranges) is delivered up to
    `window` commands late.  The ranges of one (key, voter) never overlap, and
    after the last event every frontier of a key is its highest clock, so
    every command has become stable."""
    rng = random.Random(seed)
    clocks = [[0] * keys for _ in range(n + 1)]
    seqs = [0] * (n + 1)
    out = []  # (delivery slot, creation index, event)
    for i in range(cmds):
        if keys == 1 or rng.randrange(100) < conflict_pct:
            key = 0
        else:
            key = 1 + rng.randrange(keys - 1)
        p = 1 + rng.randrange(n)
        others = rng.sample([q for q in range(1, n + 1) if q != p], fast_quorum - 1)
        seqs[p] += 1
        prop = clocks[p][key] + 1
        votes = [(p, prop, prop)]
        clocks[p][key] = prop
        commit = prop
        for q in others:
            pq = max(prop, clocks[q][key] + 1)
            votes.append((q, clocks[q][key] + 1, pq))
            clocks[q][key] = pq
            commit = max(commit, pq)
        out.append((i + rng.randrange(window + 1), len(out), ("A", key, (p, seqs[p]), commit, votes)))
        for q in range(1, n + 1):
            if clocks[q][key] < commit:
                vr = (q, clocks[q][key] + 1, commit)
                clocks[q][key] = commit
                out.append((i + rng.randrange(lag + 1), len(out), ("D", key, [vr])))
    out.sort(key=lambda e: (e[0], e[1]))
    return [e[2] for e in out]


def synth_table_streams_mk(seed, n, fast_quorum, keys, cmds, conflict_pct, lag, window, kmax=2):
    """One deterministic Tempo-shaped stream of `cmds` commands with 1..kmax
    keys each (uniform), as synth_table_streams otherwise.

    A command's first key is key 0 with probability conflict_pct percent and
    otherwise a uniform other key; its further keys are distinct uniform
    other keys.  The coordinator proposes the highest of its clocks over the
    command's keys plus one, every other fast-quorum member the higher of
    that and its own highest plus one, and each votes own + 1 .. its proposal
    on every key (fantoch_ps/src/protocol/common/table/clocks/keys/
    sequential.rs:38-57 over the command's keys); the commit clock is the
    highest proposal.  The command's attached events (one per key, ascending
    key, each with that key's quorum votes; fantoch_ps/src/protocol/
    tempo.rs:614-636) are delivered back to back, up to `window` commands
    late; per key every process below the commit clock votes up to it as a
    detached range, up to `lag` commands late."""
    rng = random.Random(seed)
    clocks = [[0] * keys for _ in range(n + 1)]
    seqs = [0] * (n + 1)
    out = []  # (delivery slot, creation index, event)
    for i in range(cmds):
        k = 1 + rng.randrange(min(kmax, keys))
        if keys == 1 or rng.randrange(100) < conflict_pct:
            first = 0
        else:
            first = 1 + rng.randrange(keys - 1)
        cmd_keys = sorted([first] + rng.sample([x for x in range(keys) if x != first], k - 1))
        p = 1 + rng.randrange(n)
        others = rng.sample([q for q in range(1, n + 1) if q != p], fast_quorum - 1)
        seqs[p] += 1
        prop = max(clocks[p][x] for x in cmd_keys) + 1
        votes = {x: [(p, clocks[p][x] + 1, prop)] for x in cmd_keys}
        for x in cmd_keys:
            clocks[p][x] = prop
        commit = prop
        for q in others:
            pq = max(prop, max(clocks[q][x] for x in cmd_keys) + 1)
            for x in cmd_keys:
                votes[x].append((q, clocks[q][x] + 1, pq))
                clocks[q][x] = pq
            commit = max(commit, pq)
        slot = i + rng.randrange(window + 1)
        for x in cmd_keys:
            out.append((slot, len(out), ("A", x, (p, seqs[p]), commit, votes[x], k)))
        for x in cmd_keys:
            for q in range(1, n + 1):
                if clocks[q][x] < commit:
                    vr = (q, clocks[q][x] + 1, commit)
                    clocks[q][x] = commit
                    out.append((i + rng.randrange(lag + 1), len(out), ("D", x, [vr])))
    out.sort(key=lambda e: (e[0], e[1]))
    return [e[2] for e in out]


# --------------------------------------------- seeded streams, canonical C6
# The purposes of the draws, as fantoch_amd/csrc/fx_table_synth.h numbers them
# (repeated here on purpose: a change on one side alone fails the CPU tests).
TS_COUNT, TS_CONFLICT, TS_FIRST, TS_COORD, TS_WINDOW, TS_KEY, TS_QUORUM, TS_LAG = 32, 33, 34, 35, 36, 40, 48, 128
_M64 = (1 << 64) - 1


def _mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def synth_rand(seed, stream, a, b):
    """fx::synth_rand (fx_synth.h): the counter RNG every draw comes from."""
    return _mix64((_mix64((_mix64(seed ^ 0x5851F42D4C957F2D) + stream) & _M64) + (a << 8) + b) & _M64)


def _with_conflicts(p, conflicts, conflict_block):
    """The conflict fields of either parameter struct."""
    conflicts = [int(c) for c in conflicts]
    if not 1 <= len(conflicts) <= 8:
        raise ValueError("1 to 8 conflict rates")
    p.num_conflicts, p.conflict_block = len(conflicts), conflict_block
    for i, c in enumerate(conflicts):
        p.conflict_pct[i] = c
    return p


def table_synth_params(seed=1, streams=1, n=5, fast_quorum=3, keys=16, cmds=100, kmax=1, conflicts=(2,), lag=6,
                       window=4, stream_base=0, conflict_block=0):
    """fx_table_synth_params.  conflicts: up to 8 conflict rates in percent;
    global stream g has conflicts[g % len] (conflict_block 0) or
    conflicts[(g // conflict_block) % len]."""
    p = _lib.TableSynthParams()
    p.seed, p.streams, p.stream_base, p.n, p.fast_quorum = seed, streams, stream_base, n, fast_quorum
    p.keys, p.cmds, p.kmax, p.window, p.lag = keys, cmds, kmax, window, lag
    return _with_conflicts(p, conflicts, conflict_block)


def table_synth_shape(params):
    """(max_steps, vmax) of fx_table_synth_shape: no stream of these
    parameters has more than max_steps events, no event more than vmax
    vote ranges.  Needs no device."""
    steps, vmax = ctypes.c_uint32(), ctypes.c_uint32()
    _lib.check(_lib.load().fx_table_synth_shape(ctypes.byref(params), ctypes.byref(steps), ctypes.byref(vmax)),
               "fx_table_synth_shape")
    return steps.value, vmax.value


def synth_table_streams_c6(params, s):
    """Stream s of fx_table_synth_generate(params), restated in plain Python:
    synth_table_streams_mk's model with every draw taken from the counter RNG
    (fantoch_amd/csrc/fx_table_synth.h) instead of random.Random.  Returns the
    event list in the tuple format of this module (nkeys only where it is not
    1, as TablePlanes.stream decodes it)."""
    p = params
    g = p.stream_base + s
    n, keys, fq = p.n, p.keys, p.fast_quorum
    nc = p.num_conflicts or 1
    conflict = p.conflict_pct[(g // p.conflict_block) % nc if p.conflict_block else g % nc]
    kcap = min(p.kmax, keys)

    def draw(i, purpose, m):
        return synth_rand(p.seed, g, i, purpose) % m

    def pick(r, taken):  # the r-th smallest id not in taken
        for c in sorted(taken):
            if c <= r:
                r += 1
        return r

    clocks = [[0] * keys for _ in range(n + 1)]
    seqs = [0] * (n + 1)
    out = []  # (delivery slot, creation index, event)
    for i in range(p.cmds):
        k = 1 + draw(i, TS_COUNT, kcap)
        cmd_keys = [0 if keys == 1 or draw(i, TS_CONFLICT, 100) < conflict else 1 + draw(i, TS_FIRST, keys - 1)]
        for j in range(1, k):
            cmd_keys.append(pick(draw(i, TS_KEY + j, keys - j), cmd_keys))
        cmd_keys.sort()
        quorum = [1 + draw(i, TS_COORD, n)]
        for j in range(1, fq):
            quorum.append(1 + pick(draw(i, TS_QUORUM + j, n - j), [q - 1 for q in quorum]))
        c = quorum[0]
        seqs[c] += 1
        prop = max(clocks[c][x] for x in cmd_keys) + 1
        votes = {x: [] for x in cmd_keys}
        commit = 0
        for q in quorum:
            pq = prop if q == c else max(prop, max(clocks[q][x] for x in cmd_keys) + 1)
            for x in cmd_keys:
                votes[x].append((q, clocks[q][x] + 1, pq))
                clocks[q][x] = pq
            commit = max(commit, pq)
        slot = i + draw(i, TS_WINDOW, p.window + 1)
        for x in cmd_keys:
            ev = ("A", x, (c, seqs[c]), commit, votes[x])
            out.append((slot, len(out), ev + (k,) if k != 1 else ev))
        for ki, x in enumerate(cmd_keys):
            for q in range(1, n + 1):
                if clocks[q][x] < commit:
                    vr = (q, clocks[q][x] + 1, commit)
                    clocks[q][x] = commit
                    out.append((i + draw(i, TS_LAG + 16 * ki + q - 1, p.lag + 1), len(out), ("D", x, [vr])))
    out.sort(key=lambda e: (e[0], e[1]))
    return [e[2] for e in out]


def synth_table_host(params, steps=None):
    """fx_table_synth_generate_host: the streams of `params` as TablePlanes,
    generated by the library on the host -- the bytes fx_table_synth_generate
    writes on the device.  steps None: the longest stream (at least 1)."""
    lib = _lib.load()
    S = int(params.streams)
    lengths = np.zeros(max(S, 1), np.uint32)
    longest = ctypes.c_uint32()
    _lib.check(lib.fx_table_synth_lengths_host(ctypes.byref(params), lengths.ctypes.data_as(_lib.u32p),
                                               ctypes.byref(longest)), "fx_table_synth_lengths_host")
    if steps is None:
        steps = max(longest.value, 1)
    p = TablePlanes(S, steps, params.n, params.keys, params.fast_quorum, lengths=lengths[:S])
    if params.kmax > 1:
        p.nkeys = np.zeros(p.plane, np.uint32)
    planes = _lib.TableSynthPlanes(p.hdr.ctypes.data, p.dot.ctypes.data, p.clock.ctypes.data, p.votes.ctypes.data,
                                   p.nkeys.ctypes.data if p.nkeys is not None else None, lengths.ctypes.data)
    _lib.check(lib.fx_table_synth_generate_host(ctypes.byref(params), ctypes.byref(planes), steps),
               "fx_table_synth_generate_host")
    return p


# ------------------------------------- seeded closed-loop groups, canonical C6
# The purposes of the group-level draws and of the delays, as
# fantoch_amd/csrc/fx_table_group_synth.h numbers them (repeated on purpose).
# Group-level draws have a = i; the draws of shard h have a = i | (h + 1) << 32
# and the TS_* purposes (TS_COORD is not drawn); a delay is drawn with the
# sender's a and purpose TG_DELAY + 8 * target shard + key index.
TG_SHARDS, TG_COORD, TG_SHARD, TG_DELAY = 37, 38, 64, 64


def table_group_synth_params(seed=1, groups=1, shards=2, smax=None, n=5, fast_quorum=3, keys=16, cmds=40, kmax=2,
                             conflicts=(2,), lag=6, window=4, msg_lag=3, group_base=0, conflict_block=0):
    """fx_table_group_synth_params.  smax None: shards.  conflicts: up to 8
    conflict rates in percent; global group G has conflicts[G % len]
    (conflict_block 0) or conflicts[(G // conflict_block) % len]."""
    p = _lib.TableGroupSynthParams()
    p.seed, p.groups, p.group_base, p.shards, p.smax = seed, groups, group_base, shards, shards if smax is None else smax
    p.n, p.fast_quorum, p.keys, p.cmds, p.kmax = n, fast_quorum, keys, cmds, kmax
    p.window, p.lag, p.msg_lag = window, lag, msg_lag
    return _with_conflicts(p, conflicts, conflict_block)


class GroupDelays(dict):
    """The delays of one generated group: (sender shard, dot, target shard,
    key) -> rounds; callable as the `delay` of pack_table_groups and of a
    closed loop."""

    def __call__(self, sender, dot, target, key):
        return self[sender, tuple(dot), target, key]


def synth_table_groups_c6(params, g):
    """Group g of fx_table_group_synth_generate(params), restated in plain
    Python: tests/table_shapes_ps.synth_table_group's model of the own events
    with every draw taken from the counter RNG
    (fantoch_amd/csrc/fx_table_group_synth.h).  Returns (own, commands,
    delays): one list of own events per shard in the tuple format of this
    module (nkeys and shards only where TablePlanes.stream decodes them), the
    map dot -> {shard: [keys]}, and the GroupDelays of the group's
    StableAtShard messages -- what pack_table_groups(groups, n, keys, delay)
    takes."""
    p = params
    G = p.group_base + g
    P, n, keys, fq = p.shards, p.n, p.keys, p.fast_quorum
    nc = p.num_conflicts or 1
    conflict = p.conflict_pct[(G // p.conflict_block) % nc if p.conflict_block else G % nc]
    kcap, scap = min(p.kmax, keys), min(p.smax, P)

    def draw(a, purpose, m):
        return synth_rand(p.seed, G, a, purpose) % m

    def pick(r, taken):  # the r-th smallest id not in taken
        for c in sorted(taken):
            if c <= r:
                r += 1
        return r

    clocks = [[[0] * keys for _ in range(n + 1)] for _ in range(P)]
    seqs = [0] * (n + 1)
    own = [[] for _ in range(P)]  # (delivery slot, creation index, event)
    commands, delays = {}, GroupDelays()
    for i in range(p.cmds):
        on = []
        for j in range(1 + draw(i, TG_SHARDS, scap)):
            on.append(pick(draw(i, TG_SHARD + j, P - j), on))
        on.sort()
        c = 1 + draw(i, TG_COORD, n)
        seqs[c] += 1
        dot = (c, seqs[c])
        cmd, votes, commit = {}, {}, 0
        for h in on:
            a = i | (h + 1) << 32
            k = 1 + draw(a, TS_COUNT, kcap)
            ck = [0 if keys == 1 or draw(a, TS_CONFLICT, 100) < conflict else 1 + draw(a, TS_FIRST, keys - 1)]
            for j in range(1, k):
                ck.append(pick(draw(a, TS_KEY + j, keys - j), ck))
            cmd[h] = sorted(ck)
            quorum = [c]
            for j in range(1, fq):
                quorum.append(1 + pick(draw(a, TS_QUORUM + j, n - j), [q - 1 for q in quorum]))
            cl = clocks[h]
            prop = max(cl[c][x] for x in cmd[h]) + 1
            for x in cmd[h]:
                votes[h, x] = []
            for q in quorum:
                pq = prop if q == c else max(prop, max(cl[q][x] for x in cmd[h]) + 1)
                for x in cmd[h]:
                    votes[h, x].append((q, cl[q][x] + 1, pq))
                    cl[q][x] = pq
                commit = max(commit, pq)
        commands[dot] = cmd
        for h in on:
            a = i | (h + 1) << 32
            k = len(cmd[h])
            slot = i + draw(a, TS_WINDOW, p.window + 1)
            for x in cmd[h]:
                ev = ("A", x, dot, commit, votes[h, x])
                ev += (k, len(on)) if len(on) != 1 else (k,) if k != 1 else ()
                own[h].append((slot, len(own[h]), ev))
            for ki, x in enumerate(cmd[h]):
                for q in range(1, n + 1):
                    if clocks[h][q][x] < commit:
                        vr = (q, clocks[h][q][x] + 1, commit)
                        clocks[h][q][x] = commit
                        own[h].append((i + draw(a, TS_LAG + 16 * ki + q - 1, p.lag + 1), len(own[h]), ("D", x, [vr])))
            for t in on:
                if t != h:
                    for ki, x in enumerate(cmd[t]):
                        delays[h, dot, t, x] = draw(a, TG_DELAY + 8 * t + ki, p.msg_lag + 1)
    own = [[e[2] for e in sorted(o, key=lambda e: (e[0], e[1]))] for o in own]
    return own, commands, delays


def table_group_synth_counts_host(params):
    """fx_table_group_synth_count_host: (lengths, longest, steps_out,
    targets_words) of the groups of `params`.  Needs no device."""
    S = int(params.groups) * int(params.shards)
    lengths = np.zeros(max(S, 1), np.uint32)
    longest, steps_out, words = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    _lib.check(_lib.load().fx_table_group_synth_count_host(ctypes.byref(params), lengths.ctypes.data_as(_lib.u32p),
                                                           ctypes.byref(longest), ctypes.byref(steps_out),
                                                           ctypes.byref(words)), "fx_table_group_synth_count_host")
    return lengths[:S], longest.value, steps_out.value, words.value


def synth_table_groups_host(params, steps=None, targets_words=None):
    """fx_table_group_synth_generate_host: the groups of `params` as
    pack_table_groups returns them -- (planes, route, targets, steps_out),
    generated by the library on the host; the bytes
    fx_table_group_synth_generate writes on the device.  steps None: the
    longest stream (at least 1); targets_words None: what the lists take."""
    lengths, longest, steps_out, words = table_group_synth_counts_host(params)
    if steps is None:
        steps = max(longest, 1)
    if targets_words is None:
        targets_words = words
    S = int(params.groups) * int(params.shards)
    lengths = np.zeros(max(S, 1), np.uint32)
    p = TablePlanes(S, steps, params.n, params.keys, params.fast_quorum, lengths=lengths[:S])
    p.nkeys = np.zeros(p.plane, np.uint32)
    p.ps = True
    route = np.zeros(p.plane, np.uint32)
    targets = np.zeros(targets_words, np.uint32)
    planes = _lib.TableGroupSynthPlanes(p.hdr.ctypes.data, p.dot.ctypes.data, p.clock.ctypes.data, p.votes.ctypes.data,
                                        p.nkeys.ctypes.data, route.ctypes.data,
                                        targets.ctypes.data if targets_words else None, lengths.ctypes.data)
    _lib.check(_lib.load().fx_table_group_synth_generate_host(ctypes.byref(params), ctypes.byref(planes), steps,
                                                              targets_words), "fx_table_group_synth_generate_host")
    return p, route, targets, steps_out
