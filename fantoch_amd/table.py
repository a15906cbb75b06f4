"""Host side of the batched Tempo TableExecutor (fx_table_*): packing streams
of TableExecutionInfo values into planes, Tempo's quorum sizes, and a
deterministic Tempo-shaped stream generator.

An event is ("A", key, (source, seq), clock, votes[, nkeys]) -- AttachedVotes
-- or ("D", key, votes) -- DetachedVotes -- with votes a list of
(voter, start, end) ranges (fantoch_ps/src/executor/table/executor.rs:110-144)
and key a dense id below `keys`.  nkeys (1 when absent) is the number of keys
of the event's command: Tempo emits one AttachedVotes per key, each with the
command's dot and clock (fantoch_ps/src/protocol/tempo.rs:614-636).
"""
import ctypes
import random

import numpy as np

from . import _lib
from ._lib import index, pack_dot, plane_words


def table_hdr(kind, nvotes, key):
    """FX_TABLE_HDR."""
    return ((int(kind) & 1) << 31) | ((int(nvotes) & 127) << 24) | (int(key) & 0xFFFFFF)


class TablePlanes:
    """Host copy of an fx_table_batch: hdr / dot / clock planes, 3 * vmax vote
    planes, lengths; nkeys is None or the extra plane of an fx_table_batch_mk."""

    def __init__(self, num_streams, steps, n, keys, vmax, lengths=None):
        self.S, self.steps, self.n, self.keys, self.vmax = int(num_streams), int(steps), int(n), int(keys), int(vmax)
        self.plane = plane_words(self.S, self.steps)
        self.hdr = np.zeros(self.plane, np.uint32)
        self.dot = np.zeros(self.plane, np.uint32)
        self.clock = np.zeros(self.plane, np.uint32)
        self.votes = np.zeros(3 * self.vmax * self.plane, np.uint32)
        self.lengths = lengths
        self.nkeys = None

    def stream(self, s):
        """Decodes stream s back into its list of events."""
        L = self.steps if self.lengths is None else int(self.lengths[s])
        out = []
        for at in index(np.arange(L), s, self.steps):
            at = int(at)
            h = int(self.hdr[at])
            key, nv = h & 0xFFFFFF, (h >> 24) & 127
            votes = [tuple(int(self.votes[(3 * j + c) * self.plane + at]) for c in range(3)) for j in range(nv)]
            if h >> 31 == _lib.FX_TABLE_ATTACHED:
                ev = ("A", key, _lib.unpack_dot(self.dot[at]), int(self.clock[at]), votes)
                if self.nkeys is not None and int(self.nkeys[at]) != 1:
                    ev += (int(self.nkeys[at]),)
                out.append(ev)
            else:
                out.append(("D", key, votes))
        return out


def _votes(ev):
    return ev[4] if ev[0] == "A" else ev[2]


def pack_table_streams(streams, n, keys):
    """streams: lists of ("A", key, (src, seq), clock, votes[, nkeys]) /
    ("D", key, votes) events.  The nkeys plane is filled when an event has
    nkeys other than 1 (fantoch_amd.device.run_table then takes the _mk entry
    points).  Raises ValueError on what the planes cannot hold: a key outside
    0..keys-1, a clock or vote at or above 2**32, more than FX_TABLE_MAX_VOTES
    ranges in an event, nkeys outside 32 bits."""
    S = len(streams)
    steps = max([len(s) for s in streams] + [1])
    vmax = max([len(_votes(ev)) for st in streams for ev in st] + [1])
    if vmax > _lib.FX_TABLE_MAX_VOTES:
        raise ValueError("an event carries %d vote ranges (at most %d)" % (vmax, _lib.FX_TABLE_MAX_VOTES))
    if not 1 <= keys <= _lib.FX_TABLE_MAX_KEYS:
        raise ValueError("keys = %d" % keys)
    p = TablePlanes(S, steps, n, keys, vmax, lengths=np.array([len(s) for s in streams], np.uint32))
    for s, st in enumerate(streams):
        if not st:
            continue
        idx = index(np.arange(len(st)), s, steps)
        for i, ev in enumerate(st):
            at = int(idx[i])
            kind, key = ev[0], int(ev[1])
            if kind not in ("A", "D") or len(ev) not in ((5, 6) if kind == "A" else (3,)):
                raise ValueError("malformed event %r" % (ev,))
            votes = _votes(ev)
            if not 0 <= key < keys:
                raise ValueError("key %d outside 0..%d" % (key, keys - 1))
            if kind == "A":
                (src, seq), clock = ev[2], int(ev[3])
                if not 0 <= clock < 1 << 32:
                    raise ValueError("clock %d does not fit 32 bits" % clock)
                if not (0 <= int(src) < 256 and 0 <= int(seq) <= _lib.FX_SEQ_MASK):
                    raise ValueError("dot %r does not fit the packed form" % ((src, seq),))
                p.dot[at] = pack_dot(src, seq)
                p.clock[at] = clock
                nk = int(ev[5]) if len(ev) == 6 else 1
                if not 0 <= nk < 1 << 32:
                    raise ValueError("nkeys %d does not fit 32 bits" % nk)
                if nk != 1 and p.nkeys is None:
                    p.nkeys = np.ones(p.plane, np.uint32)
                if p.nkeys is not None:
                    p.nkeys[at] = nk
            p.hdr[at] = table_hdr(_lib.FX_TABLE_ATTACHED if kind == "A" else _lib.FX_TABLE_DETACHED, len(votes), key)
            for j, vr in enumerate(votes):
                for c in range(3):
                    if not 0 <= int(vr[c]) < 1 << 32:
                        raise ValueError("vote range %r does not fit 32 bits" % (vr,))
                    p.votes[(3 * j + c) * p.plane + at] = int(vr[c])
    return p


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
