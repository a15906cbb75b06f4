"""Batches for the KV stage (fx_kv_execute), shared by the CPU tests of the
host twin and the GPU tests: each is small, and sits on an edge of the kernel
(the 64-row chunk, the LDS / HBM table tiers, the op slots, the order word's
flag).  A stream is a dict: order (arrival rows in execution order), keys_of /
ops_of (by arrival row), optionally nexec (when it is not len(order)) and err
(the status the stream must end with; such a stream writes nothing else).
Everything a call must not read or write holds the byte 0xA5."""
import random

import numpy as np

from fantoch_amd import _lib
from fantoch_amd import kv as K

import kv_ref
import table_ref as R
import table_ref_mk as RM
from fantoch_amd import table as ft

A5 = 0xA5A5A5A5
ABOVE = _lib.FX_KV_ONCHIP_KEYS + 88  # keys of the HBM tier: entries k and k + 64 .. share an owner lane
G, D = K.kv_op(K.GET), K.kv_op(K.DELETE)


def P(v):
    return K.kv_op(K.PUT, v)


class Case:
    def __init__(self, name, streams, keys, omax, key_high=0, flag_every=0, steps=None):
        self.name, self.streams, self.keys, self.omax = name, streams, keys, omax
        self.S = len(streams)
        self.steps = steps or max([len(st["keys_of"]) for st in streams] + [1])
        self.key_mask = 0x00FFFFFF if key_high else 0xFFFFFFFF
        pw = self.plane = _lib.plane_words(self.S, self.steps)
        self.order, self.key = np.full(pw, A5, np.uint32), np.full(pw, A5, np.uint32)
        self.ops = np.full(omax * pw, A5, np.uint32)
        self.nexec = np.zeros(self.S, np.uint32)
        for s, st in enumerate(streams):
            self.nexec[s] = st.get("nexec", len(st["order"]))
            for k, a in enumerate(st["order"]):
                flag = _lib.FX_ORDER_SCC_START if flag_every and k % flag_every == 0 else 0
                self.order[_lib.index(k, s, self.steps)] = a | flag
            for a, (key, ops) in enumerate(zip(st["keys_of"], st["ops_of"])):
                at = int(_lib.index(a, s, self.steps))
                self.key[at] = key | key_high
                for j in range(omax):
                    self.ops[j * pw + at] = ops[j] if j < len(ops) else K.kv_op(K.EMPTY)

    def run_host(self):
        return K.run_kv_host(self.order, self.nexec, self.key, self.ops, self.S, self.steps, self.keys, self.omax,
                             self.key_mask, fill=0xA5)

    def check(self, res):
        """res (a KvResult whose outputs started as 0xA5) against the restatement."""
        assert res.status == 0
        touched = np.zeros(self.plane, bool)
        for s, st in enumerate(self.streams):
            if st.get("err"):
                assert int(res.err[s]) == st["err"], (self.name, s, int(res.err[s]))
                assert np.all(res.store[s] == A5) and np.all(res.mon_off[s] == A5), (self.name, s)
                continue
            ops_of = [[op for op in ops if K.op_kind(op) != K.EMPTY] for ops in st["ops_of"]]
            kv_ref.check_stream(res, s, st["order"], st["keys_of"], ops_of)
            touched[_lib.index(np.asarray(st["order"], np.int64), s, self.steps)] = True
            used = int(res.mon_off[s, self.keys])
            rest = _lib.index(np.arange(used, self.steps), s, self.steps)
            assert np.all(res.monitor[rest] == A5), (self.name, s)
        for j in range(self.omax):  # rows that were not executed, pad rows and pad streams: untouched
            assert np.all(res.result[j * self.plane:(j + 1) * self.plane][~touched] == A5), (self.name, j)
        pad = np.ones(self.plane, bool)
        for s in range(self.S):
            if not self.streams[s].get("err"):
                pad[_lib.index(np.arange(self.steps), s, self.steps)] = False
        assert np.all(res.monitor[pad] == A5), self.name


def stream(order, keys_of, ops_of, **kw):
    return dict(order=list(order), keys_of=list(keys_of), ops_of=[list(o) for o in ops_of], **kw)


def rand_ops(rng, omax):
    n = rng.choice([1, 1, 1, omax, rng.randrange(0, omax + 1)])
    return [rng.choice([G, G, D, P(rng.randrange(1, 1 << 30)), P(rng.randrange(1, 9))]) for _ in range(n)]


def rand_stream(rng, rows, nexec, keys, omax):
    """`rows` arrival rows of which a random `nexec` execute, in a random order."""
    return stream(rng.sample(range(rows), nexec), [rng.randrange(keys) for _ in range(rows)],
                  [rand_ops(rng, omax) for _ in range(rows)])


def chunk_edges(S, keys, omax=1):
    rng = random.Random(1000 * S + keys)
    counts = [0, 1, 63, 64, 65, 129]
    return Case("edges S%d k%d" % (S, keys), [rand_stream(rng, 131, counts[s % 6], keys, omax) for s in range(S)],
                keys, omax, flag_every=3)


def patterns(keys):
    spread = [(k * 73) % keys for k in range(64)]  # 64 distinct keys; above 64 keys some share an owner lane
    assert len(set(spread)) == 64
    k1, k2 = keys - 1, keys // 2
    cyc = [[P(7)], [G], [D]]
    sts = [
        # 64 rows of one key, PUT / GET / DELETE in turn
        stream(range(64), [k1] * 64, [[P(100 + i)] if i % 3 == 0 else cyc[i % 3] for i in range(64)]),
        # 64 rows on 64 distinct keys, then each read back in the next chunk
        stream(range(128), spread + spread[::-1], [[P(1 + i)] for i in range(64)] + [[G]] * 64),
        # a PUT at row 63 read by a GET at row 64
        stream(range(65), [k2] * 65, [[G]] * 63 + [[P(4242)], [G]]),
        # DELETE then GET; PUT over PUT
        stream(range(6), [k1, k1, k1, k2, k2, k2], [[P(5)], [D], [G], [P(6)], [P(8)], [G]]),
        # the same across a chunk edge: the table carries the value
        stream(range(130), [k1] * 130, [[P(5)]] + [[G]] * 63 + [[D]] + [[G]] * 63 + [[P(9)], [P(10)]]),
        # executed in another order than the rows arrived
        stream(range(69, -1, -1), [spread[i % 7] for i in range(70)], [[P(1 + i)] if i % 2 else [G] for i in range(70)]),
    ]
    return Case("patterns k%d" % keys, sts, keys, 1, flag_every=2)


def op_slots(omax, keys=64):
    rng = random.Random(omax)
    full = [G, P(11), G, D][:omax]
    sts = [
        stream(range(5), [3, 3, 3, 3, 3], [[P(1)], full, [], [G] * omax, full]),  # mixed counts, a zero-op partial
        stream(range(66), [5] * 66, [full if i % 2 else [P(20 + i)] for i in range(66)]),
        rand_stream(rng, 140, 140, 3, omax),
        rand_stream(rng, 70, 40, keys, omax),
    ]
    return Case("slots o%d k%d" % (omax, keys), sts, keys, omax)


def monitor_case(keys):
    # read-only partials leave no trace; one key's order runs over three chunks
    rows = 150
    ops = [[G] if i % 4 == 1 else [G, G] if i % 4 == 2 else [P(1 + i)] if i % 4 == 3 else [D] for i in range(rows)]
    sts = [stream(range(rows), [keys - 2 if i % 3 else 1 for i in range(rows)], ops),
           stream(range(70), [0] * 70, [[G]] * 70)]
    return Case("monitor k%d" % keys, sts, keys, 2, key_high=0x83000000)


def errors(keys):
    """Every per-stream status, between streams that run."""
    rng = random.Random(keys)
    steps = 72
    ok = lambda: rand_stream(rng, steps, 70, min(keys, 9), 2)
    E, O = _lib.FX_ERR_INVALID_ARG, _lib.FX_ERR_ORDER_OVERFLOW
    base = ok()
    sts = [
        ok(),
        dict(base, nexec=steps + 1, err=O),
        dict(ok(), order=list(range(69)) + [steps], err=E),                  # an arrival row >= steps
        dict(ok(), order=list(range(69)) + [0x7FFFFFFF], err=E),
        ok(),
        dict(stream(range(70), [1] * 68 + [keys, 1], [[G]] * 70), err=E),    # a key >= keys
        dict(stream(range(70), [1] * 70, [[G]] * 66 + [[P(0)]] + [[G]] * 3), err=E),   # a PUT of value 0
        dict(stream(range(70), [1] * 70, [[P(3)]] * 69 + [[K.kv_op(K.EMPTY), G]]), err=E),  # used after EMPTY
        dict(stream(range(2), [0, 0], [[G, P(0)], [G]]), err=E),
        ok(),
    ]
    return Case("errors k%d" % keys, sts, keys, 2, steps=steps)


def all_cases():
    out = [chunk_edges(S, 5) for S in (1, 64, 65)] + [chunk_edges(65, ABOVE)]
    for keys in (64, ABOVE):
        out += [patterns(keys), monitor_case(keys), errors(keys)]
    out += [op_slots(1), op_slots(4), op_slots(4, ABOVE)]
    return out


# ------------------------------------------------------------------ behind the table executor
N, FQ, THR, KEYS, CMDS, LAG, WINDOW = 5, 3, 3, 4, 40, 6, 4


def replicas(base, seed):
    out = [base]
    for r in range(3):
        ev = list(base)
        random.Random(1000 * seed + r).shuffle(ev)
        out.append(ev)
    return out


def command_ops(streams, seed):
    """One partial per (dot, key) of the streams' commands, the same at every replica."""
    rng = random.Random(seed)
    ops = {}
    for ev in streams[0]:
        if ev[0] == "A":
            ops[(ev[2], ev[1])] = rand_ops(rng, 2)
    return ops


def table_batch(mk):
    """[(events, restatement, keys_of, ops_of)] per stream: 4 conflict rates x (base + 3 shuffles)."""
    out = []
    # multi-key: most shuffles of a whole event list leave the executor waiting at the end of the stream (a
    # command's later partial arrives after the earlier one executed and starts a command of its own: C13);
    # over seeds 0..39 and these four rates 418 of 480 shuffles do, none disagrees, and (rate 0, seed 29) is
    # the one combination whose three shuffles all execute every command, which check_precondition asserts
    for seed, conflict in ((29, 0),) if mk else enumerate((0, 10, 50, 100)):
        if mk:
            base = ft.synth_table_streams_mk(seed, N, FQ, KEYS, CMDS, conflict, LAG, WINDOW, kmax=2)
        else:
            base = ft.synth_table_streams(seed, N, FQ, KEYS, CMDS, conflict, LAG, WINDOW)
        reps = replicas(base, seed)
        ops = command_ops(reps, seed)
        for ev in reps:
            ref = (RM if mk else R).run_stream(ev, N, THR, KEYS)
            keys_of = [e[1] for e in ev]
            ops_of = [ops[(e[2], e[1])] if e[0] == "A" else [] for e in ev]
            out.append((ev, ref, keys_of, ops_of))
    return out


def check_precondition(batch):
    """On the restatement alone: no stream has an error, every command executes, the replicas agree."""
    for g in range(0, len(batch), 4):
        mons = []
        for ev, ref, keys_of, ops_of in batch[g:g + 4]:
            assert ref["err"] == 0 and ref["nexec"] == sum(e[0] == "A" for e in ev)
            mons.append((kv_ref.run(ref["order"], keys_of, ops_of)[2], [e[2] if e[0] == "A" else None for e in ev]))
        for mon, dots in mons[1:]:
            assert kv_ref.first_difference(mons[0][0], mons[0][1], mon, dots, KEYS) is None
