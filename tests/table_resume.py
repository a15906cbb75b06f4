"""Shared pieces of the tests of the resumable table executor
(fx_table_advance, fantoch_amd.device.TableSession) and of the closed loop
over groups of shard executors (fantoch_amd.table.run_table_groups): a
session backed by the restatement, the closed loop restated on the CPU, the
prefix results of a stream, and the streams the GPU cut tests use with what
the restatement says they hold at their cuts."""
import functools

import numpy as np

from fantoch_amd import _lib
from fantoch_amd import table as ft

import table_ref as R
import table_ref_mk as RM
import table_ref_ps as RP
import table_shapes_ps as TP
from table_shapes import quorum_sizes

SINGLE, MK, PS = _lib.FX_TABLE_KIND_SINGLE, _lib.FX_TABLE_KIND_MK, _lib.FX_TABLE_KIND_PS
RUN = {SINGLE: R.run_stream, MK: RM.run_stream, PS: RP.run_stream}
NONE = _lib.FX_RELEASE_NONE


class RefResult:
    pass


class RefSession:
    """What fantoch_amd.device.TableSession is to run_table_groups, over the
    restatement (tests/table_ref_ps.py Stream): advance(planes) feeds every
    stream its new rows and returns the cumulative output planes."""

    def __init__(self, S, steps, n, keys, vmax, stability_threshold, kind, execute_at_commit=False):
        assert kind == PS
        self.S, self.steps, self.keys = S, steps, keys
        self.sims = [RP.Stream(n, stability_threshold, keys, vmax, execute_at_commit) for _ in range(S)]
        self.fed = [0] * S
        self.calls = 0

    def advance(self, planes):
        assert (planes.S, planes.steps, planes.keys) == (self.S, self.steps, self.keys) and planes.ps
        self.calls += 1
        res = RefResult()
        pw = planes.plane
        res.order = np.zeros(pw, np.uint32)
        res.release = np.full(pw, NONE, np.uint32)
        res.stable_sent = np.full(pw, NONE, np.uint32)
        res.nexec, res.err = np.zeros(self.S, np.uint32), np.zeros(self.S, np.uint32)
        res.stable_clock = np.zeros((self.S, self.keys), np.uint32)
        for s, sim in enumerate(self.sims):
            assert int(planes.lengths[s]) >= self.fed[s]
            for ev in planes.stream(s, self.fed[s]):
                sim.feed(ev)
            self.fed[s] = int(planes.lengths[s])
            ref = sim.result()
            res.nexec[s], res.err[s] = ref["nexec"], ref["err"]
            res.stable_clock[s] = ref["stable"]
            res.order[_lib.index(np.arange(ref["nexec"]), s, self.steps)] = \
                np.array(ref["order"], np.uint32) | np.uint32(_lib.FX_ORDER_SCC_START)
            for name, plane in (("release", res.release), ("sent", res.stable_sent)):
                for a, step in ref[name].items():
                    plane[int(_lib.index(a, s, self.steps))] = step
        return res


def hashed_delay(sender, dot, target, key):
    """0..3 rounds, fixed by the message."""
    return (dot[0] * 7 + dot[1] * 13 + target * 5 + key * 3 + sender) % 4


def closed_loop(own, commands, n, thr, keys, delay=None):
    """One group's closed loop restated over table_ref_ps.Stream, event by
    event.  Returns (streams as handled, results)."""
    G = len(own)
    sims = [RP.Stream(n, thr, keys) for _ in range(G)]
    streams = [[] for _ in range(G)]
    due = [[] for _ in range(G)]
    nsent, t = 0, 0
    while any(sims[g].err == 0 and (t < len(own[g]) or due[g]) for g in range(G)):
        for g in range(G):
            if sims[g].err:
                due[g] = []
                continue
            now = sorted(m for m in due[g] if m[0] <= t)
            due[g] = [m for m in due[g] if m[0] > t]
            for ev in [("S", x, dot) for _, _, x, dot in now] + ([own[g][t]] if t < len(own[g]) else []):
                before = set(sims[g].ex.sent)
                streams[g].append(ev)
                if sims[g].err == 0:
                    sims[g].feed(ev)
                for a in sorted(set(sims[g].ex.sent) - before):
                    dot = streams[g][a][2]
                    for h in sorted(commands[dot]):
                        if h != g:
                            for x in sorted(commands[dot][h]):
                                lag = delay(g, dot, h, x) if delay else 0
                                due[h].append((t + 1 + lag, nsent, x, dot))
                                nsent += 1
        t += 1
    return streams, [s.result() for s in sims]


FIELDS = ("order", "release", "sent", "nexec", "err", "stable")


def own_events(streams):
    return [[ev for ev in st if ev[0] != "S"] for st in streams]


def prefixes(kind, stream, n, thr, keys, execute_at_commit=False):
    """(nexec, err, stable clocks) the restatement reports after each prefix
    of the stream, prefix 0 included: one pass over table_ref_ps.Stream, which
    the streams used here (no errors before the last event) run through as
    through their own kind's restatement -- checked for the whole stream."""
    sim = RP.Stream(n, thr, keys, None, execute_at_commit)
    out = [(0, 0, [0] * keys)]
    for ev in stream:
        sim.feed(ev)
        ref = sim.result()
        out.append((ref["nexec"], ref["err"], ref["stable"]))
    whole = RUN[kind](list(stream), n, thr, keys, execute_at_commit=execute_at_commit)
    assert (whole["nexec"], whole["err"], whole["stable"]) == out[-1]
    return out


def op_states(ex):
    """The states of the live partials of a table_ref_mk / table_ref_ps Executor."""
    in_table = {id(p) for t in ex.tables.values() for p in t.ops.values()}
    tried = {id(p) for ps in ex.tried.values() for p in ps}
    out = set()
    for ps in ex.live.values():
        for p in ps:
            out.add("table" if id(p) in in_table else "told" if p.told else "tried" if id(p) in tried else "queued")
    return out


def coverage(stream, n, thr, keys):
    """What the restatement holds after each event but the last: the rows
    whose drain leaves a message on to_executors, the rows after which ops are
    in all four states, and the rows after which a buffered pair is alive."""
    sim = RP.Stream(n, thr, keys)
    left, four, pairs = [], [], []
    for r, ev in enumerate(stream[:-1]):
        assert sim.feed(ev) == 0
        if sim.ex.to_executors:
            left.append(r)
        if op_states(sim.ex) == {"table", "queued", "tried", "told"}:
            four.append(r)
        if sim.ex.npairs:
            pairs.append(r)
    return left, four, pairs


# the streams of the cut tests: kind -> (n, f, stream); seeds chosen on the CPU
# so that coverage() holds what test_table_resume_cpu.py asserts of them
CUT_N, CUT_F, CUT_KEYS = 3, 1, 16


@functools.lru_cache(maxsize=None)
def cut_stream(kind):
    fq, _, thr = quorum_sizes(CUT_N, CUT_F, False)
    if kind == SINGLE:
        st = ft.synth_table_streams(7, CUT_N, fq, CUT_KEYS, 90, 50, 6, 4)
    elif kind == MK:
        st = ft.synth_table_streams_mk(0, CUT_N, fq, CUT_KEYS, 55, 100, 6, 6, 3)  # lag 6, window 6, kmax 3
    else:  # two shards, kmax 3, msg_lag 3; shard 0's stream
        st = TP.synth_table_group(1, 2, CUT_N, fq, thr, CUT_KEYS, 56, 100, 4, 0, 3, 2, 3)[0][0]
    return tuple(st), thr
