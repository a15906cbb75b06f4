"""Batches for the pending stage (fx_pending_aggregate), shared by the CPU
tests of the host twin and the GPU tests: each is small and sits on an edge of
the kernel (the 64-row chunk, the 64 builders of the ONCHIP tier, the buckets
of the HBM tier).  A stream is a dict: order (arrival rows in execution order),
rifl_of / count_of (by arrival row), optionally nexec (when it is not
len(order)) and err (the status the stream must end with).  Everything a call
must not read or write holds the byte 0xA5."""
import random

import numpy as np

from fantoch_amd import _lib
from fantoch_amd import pending as P

import pending_ref

A5 = 0xA5A5A5A5
E, C, O = _lib.FX_ERR_INVALID_ARG, _lib.FX_ERR_CAPACITY, _lib.FX_ERR_ORDER_OVERFLOW
ONCHIP, HBM = P.ONCHIP, P.HBM


def rifl(seq, src=1):
    return (src << 24) | seq


class Case:
    """tiers: the tiers the case runs at (None = fx_pending_run, which no stream leaves with FX_ERR_CAPACITY and
    whose own status is FX_OK whatever the streams' are)."""

    def __init__(self, name, streams, tiers=(ONCHIP, HBM, None), count_high=0, process=0, flag_every=0, steps=None):
        self.name, self.streams, self.tiers, self.process = name, streams, tiers, process
        self.S = len(streams)
        self.steps = steps or max([len(st["rifl_of"]) for st in streams] + [1])
        self.count_mask = 0xFF if count_high else 0xFFFFFFFF
        pw = self.plane = _lib.plane_words(self.S, self.steps)
        self.order, self.rifl, self.count = (np.full(pw, A5, np.uint32) for _ in range(3))
        self.nexec = np.zeros(self.S, np.uint32)
        for s, st in enumerate(streams):
            self.nexec[s] = st.get("nexec", len(st["order"]))
            for k, a in enumerate(st["order"]):
                flag = _lib.FX_ORDER_SCC_START if flag_every and k % flag_every == 0 else 0
                self.order[_lib.index(k, s, self.steps)] = a | flag
            for a, (r, c) in enumerate(zip(st["rifl_of"], st["count_of"])):
                at = int(_lib.index(a, s, self.steps))
                self.rifl[at], self.count[at] = r, c | count_high

    def run_host(self, tier):
        return P.run_pending_host(self.order, self.nexec, self.rifl, self.count, self.S, self.steps, self.count_mask,
                                  self.process, HBM if tier is None else tier, fill=0xA5)

    def restated(self, s, tier):
        st = self.streams[s]
        return pending_ref.run(st["order"], st["rifl_of"], st["count_of"], self.steps, st.get("nexec"), self.process,
                               _lib.FX_PENDING_ONCHIP_LIVE if tier == ONCHIP else None)

    def check(self, res, tier, only=None):
        """res (a PendingResult whose outputs started as 0xA5) against the restatement; only: the streams that ran."""
        assert res.status == 0
        pw, steps = self.plane, self.steps
        want = {name: np.full(len(getattr(res, name)), A5, np.uint32) for name in P.NAMES}
        for s, st in enumerate(self.streams):
            if only is not None and s not in only:
                continue
            ref = self.restated(s, tier)
            if "err" in st:  # the stream stops where the shape means it to
                expect = st["err"] if isinstance(st["err"], int) else st["err"][tier]
                assert ref["err"] == expect, (self.name, s, ref["err"])
            want["err"][s], want["nready"][s], want["nopen"][s] = ref["err"], len(ref["ready"]), ref["nopen"]
            for a, h in ref["head"].items():
                want["head"][_lib.index(a, s, steps)] = h
            for (j, h), a in ref["part"].items():
                want["part"][j * pw + _lib.index(h, s, steps)] = a
            for h, i in ref["index"].items():
                want["index"][_lib.index(h, s, steps)] = i
            for i, h in enumerate(ref["ready"]):
                want["ready"][_lib.index(i, s, steps)] = h
        for name in P.NAMES:
            got = getattr(res, name)
            assert np.array_equal(got, want[name]), \
                "%s: %s differs at word %d" % (self.name, name, int(np.flatnonzero(got != want[name])[0]))


def stream(rows, **kw):
    """rows: [(rifl, count)] by arrival row, executed in that order unless `order` says otherwise."""
    rows = list(rows)
    st = dict(order=list(range(len(rows))), rifl_of=[r for r, _ in rows], count_of=[c for _, c in rows])
    st.update(kw)
    return st


def singles(n, base):
    return [(rifl(base + i, 2), 1) for i in range(n)]


def rand_stream(rng, rows, nexec):
    """1- to 3-key commands, a random subset nobody waits for, executed nearly in arrival order."""
    cmds, a = [], 0
    while a < rows:
        c = min(rng.choice([1, 1, 2, 2, 3]), rows - a)
        cmds.append((rifl(len(cmds), 1 + len(cmds) % 3), 0 if rng.random() < 0.2 else c, c))
        a += c
    parts = [(r, c) for r, c, n in cmds for _ in range(n)]
    rng.shuffle(parts)
    order = sorted(range(rows), key=lambda i: i + rng.randrange(24))
    return stream(parts, order=order[:nexec], err=0)


def chunk_edges(S):
    rng = random.Random(77 * S)
    counts = [129, 0, 1, 63, 64, 65]  # (a single stream, S = 1, runs three chunks beside 63 pad lanes)
    return Case("edges S%d" % S, [rand_stream(rng, 131, counts[s % 6]) for s in range(S)], flag_every=3)


def pairs_and_wide():
    X, Y = rifl(7), rifl(8)
    eight = {10, 40, 63, 64, 70, 127, 128, 140}
    sts = [
        stream([(X, 2), (X, 2)] + singles(62, 100), err=0),                      # lanes 0 and 1
        stream([(X, 2)] + singles(62, 100) + [(X, 2)], err=0),                   # lanes 0 and 63
        stream(singles(63, 100) + [(X, 2), (X, 2)] + singles(3, 200), err=0),    # rows 63 and 64
        stream(singles(5, 100) + [(X, 8)] * 8 + singles(5, 200), err=0),         # 8 keys inside one chunk
        stream([(X, 8) if a in eight else (rifl(100 + a, 3), 1) for a in range(150)], err=0),  # over three chunks
        # several commands of one chunk, completing out of head order: C, B, A
        stream([(X, 2), (Y, 2), (rifl(9), 3), (rifl(9), 3), (rifl(9), 3), (Y, 2)] + singles(3, 100) + [(X, 2)], err=0),
        # count-1 rows between the partials of an open command, one of them with its rifl (a command of its own)
        stream([(X, 3), (X, 1), (X, 3)] + singles(70, 100) + [(X, 3), (rifl(51), 1)], err=0),
    ]
    return Case("pairs and wide", sts, flag_every=2)


def reuse():
    X, Y = rifl(7), rifl(8)
    sts = [
        # within one chunk: twice complete, then a third command left open
        stream([(X, 2)] * 5 + singles(3, 100), err=0),
        # across chunks: the third command completes in the next chunk, a fourth runs in the third
        stream([(X, 2)] * 5 + singles(59, 100) + [(X, 2)] + singles(65, 200) + [(X, 2), (X, 2)], err=0),
        # the count changes where a command of the rifl completed: a new command, not a mismatch
        stream([(X, 2), (X, 2), (X, 3), (Y, 2), (X, 3), (X, 3), (X, 2)] + singles(60, 100) + [(X, 2), (Y, 2)], err=0),
        # a builder from an earlier chunk completes and its rifl starts again, twice, in one chunk
        stream([(X, 3)] + singles(64, 100) + [(X, 3), (X, 3), (X, 3), (X, 3), (X, 3), (X, 3), (X, 3)], err=0),
    ]
    return Case("rifl reuse", sts)


def live(n, tail=()):
    """n commands of two partials, every first before any second (the seconds in reverse), then `tail`."""
    return [(rifl(i), 2) for i in range(n)] + [(rifl(i), 2) for i in reversed(range(n))] + list(tail)


def capacity():
    X = rifl(500)
    sts = [
        stream(live(64), err=0),                                                  # exactly 64 live builders
        stream(live(65), err={ONCHIP: C, HBM: 0, None: 0}),                       # the 65th stops the ONCHIP tier
        stream(singles(7, 900), err=0),
        # 63 live; then in one chunk X opens (64), completes, rifl 600 opens (64), builder 0 completes, X opens
        # again (64): never 65, whatever the order in which the chunk's rifls are served
        stream([(rifl(i), 2) for i in range(63)] + singles(1, 900) +
               [(X, 2), (X, 2), (rifl(600), 2), (rifl(0), 2), (X, 2)], err=0),
        # as before, but nothing completes between: the second opening is the 65th builder
        stream([(rifl(i), 2) for i in range(63)] + singles(1, 900) +
               [(X, 2), (rifl(600), 2), (rifl(0), 2)], err={ONCHIP: C, HBM: 0, None: 0}),
        # slots freed in one chunk are taken again in the next
        stream(live(64, [(rifl(700 + i), 2) for i in range(64)] + singles(3, 900)), err=0),
    ]
    return Case("capacity", sts)


def colliding(n, buckets, bucket=1):
    out, seq = [], 0
    while len(out) < n:
        seq += 1
        if _lib.pending_bucket(rifl(seq), buckets) == bucket:
            out.append(rifl(seq))
    return out


def hbm_buckets():
    X = rifl(7)
    steps = 192
    buckets = _lib.pending_buckets(steps)
    assert buckets == 3
    same = colliding(70, buckets)
    last = colliding(70, buckets, buckets - 1)  # the walk wraps round to bucket 0
    sts = [
        # more than 64 live rifls of one bucket: the look-up walks into the next
        stream([(r, 2) for r in same] + singles(50, 100) + [(r, 2) for r in reversed(same)], err=0),
        stream([(r, 2) for r in last] + singles(2, 100) + [(r, 2) for r in last[3:]], err=0),
        # a completed entry and a live one of the same rifl in one bucket
        stream([(X, 2)] + singles(63, 100) + [(X, 2), (X, 2)] + singles(62, 200) + [(X, 2), (X, 2)], err=0),
    ]
    return Case("hbm buckets", sts, tiers=(HBM, None), steps=steps)


def errors():
    """Every status, between streams that run."""
    rng = random.Random(5)
    steps = 140
    ok = lambda: rand_stream(rng, steps, 130)
    X = rifl(7)
    sts = [
        ok(),
        stream(singles(5, 100) + [(X, 9)] + singles(5, 200), err=E),                       # count 9
        ok(),
        stream(singles(5, 100) + [(X, 2), (rifl(9), 2), (X, 3)] + singles(5, 200), err=E),  # mismatch, same chunk
        stream([(X, 3), (X, 3)] + singles(70, 100) + [(rifl(9), 2), (X, 2), (rifl(9), 2)], err=E),  # a later chunk
        ok(),
        dict(stream(singles(70, 100)), order=list(range(66)) + [steps, 67], err=E),        # an arrival row >= steps
        dict(stream(singles(70, 100)), order=list(range(3)) + [0x7FFFFFFF], err=E),
        dict(ok(), nexec=steps + 1, err=O),
        ok(),
    ]
    return Case("errors", sts, steps=steps)


def masked():
    """A plane of FX_TABLE_PS_WORD as it is; process 2 ignores the other sources."""
    rows = []
    for i in range(40):
        src = 1 + i % 3
        rows += [(rifl(i, src), 1 + i % 2)] * (1 + i % 2)
    sts = [stream(rows, err=0), stream(rows[::-1], err=0)]
    return [Case("ps words", sts, count_high=3 << 8), Case("process 2", sts, count_high=1 << 8, process=2)]


def all_cases():
    return [chunk_edges(S) for S in (1, 64, 65)] + [pairs_and_wide(), reuse(), capacity(), hbm_buckets(), errors()] + \
        masked()
