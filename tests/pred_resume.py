"""Sessions of the predecessors executor (fx_pred_advance): the partitions of a
case's streams into calls, what every call must leave (pred_ref over the rows
handed over so far at the tier's limits, over buffers of 0xA5 bytes), the
hand-built streams that carry registrations across a cut, and the driver that
feeds sessions call by call and compares them.  Shared by the CPU and the GPU
tests (test infrastructure; no test in here)."""
import sys

import numpy as np

from fantoch_amd import _lib
from fantoch_amd import pred as fpred

import pred_edges as E
import pred_ref as R

FILL, A5 = E.FILL, E.A5
SMALL, LDS, HBM = R.SMALL, R.LDS, R.HBM
NAMES = fpred.NAMES
INVALID = _lib.FX_ERR_INVALID_ARG


def batch(case):
    """(planes, clock_lo, clock_hi, ndeps) as a session takes them (ndeps None: counted by the header)."""
    planes, clo, chi, nd = case.packed()
    return planes, clo, chi, (None if case.header_nd else nd)


def lengths_of(case):
    return np.asarray(case.packed()[0].lengths, np.uint32)


class Expect:
    """The planes after each call: pred_ref.run(stream[:len], n, tier_limits(tier, n, dmax), at_commit) for every
    stream, laid over 0xA5 fill as Case.planes_of lays it.  pred_ref handles one Add at a time, so a run over a
    longer prefix is the run over the shorter one continued: the graphs are kept and fed the new rows, and the
    planes get the new order rows and release steps (lens must not decrease)."""

    def __init__(self, case, tier, at_commit=False):
        planes = case.packed()[0]
        self.case, self.steps = case, planes.steps
        self.out = dict(order=np.full(planes.plane, A5, np.uint32), release=np.full(planes.plane, A5, np.uint32),
                        nexec=np.full(case.S, A5, np.uint32), err=np.full(case.S, A5, np.uint32))
        lim = case.limits(tier)
        assert lim is not None
        self.g = [R.Graph(case.n, lim, at_commit) for _ in range(case.S)]
        self.done, self.err, self.k = [0] * case.S, [0] * case.S, [0] * case.S

    def after(self, lens):
        old = sys.getrecursionlimit()
        sys.setrecursionlimit(max(old, 40000))
        try:
            for s, st in enumerate(self.case.streams):
                g, L = self.g[s], min(int(lens[s]), len(st))
                assert L >= self.done[s]
                try:
                    while self.done[s] < L and not self.err[s]:
                        rec = self.done[s]
                        add = st[rec]
                        g.step = rec
                        self.done[s] += 1
                        g.add(tuple(add[0]), rec, tuple(add[3]), set(tuple(d) for d in add[1]))
                except R.Stop as e:
                    self.err[s] = e.err
                self.done[s] = L
                new = g.order[self.k[s]:]
                if new:
                    rows = np.asarray(new, np.int64)
                    self.out["order"][_lib.index(np.arange(self.k[s], len(g.order)), s, self.steps)] = \
                        rows.astype(np.uint32) | np.uint32(R.SCC_START)
                    self.out["release"][_lib.index(rows, s, self.steps)] = \
                        np.asarray([g.release[r] for r in new], np.uint32)
                    self.k[s] = len(g.order)
                self.out["nexec"][s], self.out["err"][s] = len(g.order), self.err[s]
        finally:
            sys.setrecursionlimit(old)
        return self.out


def expected_after(case, lens, tier, at_commit=False):
    """order, release, nexec, err after the call that brought the streams to `lens` rows (a fresh computation:
    Case.planes_of over pred_ref.run of the prefixes)."""
    lim = case.limits(tier)
    return case.planes_of({s: R.run(st[:min(int(l), len(st))], case.n, lim, at_commit)
                           for s, (st, l) in enumerate(zip(case.streams, lens))})


# ------------------------------------------------------------------ partitions: a list of lengths per call
def capped(case, cut):
    return np.minimum(lengths_of(case), np.uint32(cut)).astype(np.uint32)


def one_call(case):
    return [lengths_of(case).copy()]


def longest(case):
    return max([len(st) for st in case.streams] + [1])


def row_per_call(case):
    return [capped(case, c) for c in range(1, longest(case) + 1)]


def cuts_of(case, k=4):
    """A call at every multiple of k rows, then the rest."""
    return [capped(case, c) for c in range(k, longest(case), k)] + [lengths_of(case).copy()]


def cut_pairs(case, seed):
    """Three calls; stream s is cut at its own two rows 0 <= c1 <= c2 <= L, so a call moves different streams by
    different amounts.  Every fifth stream has c1 == c2 (its second call is empty), every seventh c1 == 0, every
    eleventh c2 == L (its last call is empty)."""
    rng = np.random.default_rng(seed)
    L = np.asarray([len(st) for st in case.streams], np.int64)
    c = np.sort(np.stack([rng.integers(0, L + 1), rng.integers(0, L + 1)]), axis=0)
    s = np.arange(case.S)
    c[0] = np.where(s % 7 == 3, 0, c[0])
    c[1] = np.where(s % 11 == 5, L, c[1])
    c[0] = np.where(s % 5 == 1, c[1], c[0])
    return [c[0].astype(np.uint32), c[1].astype(np.uint32), lengths_of(case).copy()]


def stop_row(case, s, tier, at_commit=False):
    """The row where pred_ref says stream s stops at the tier (None: it does not)."""
    return case.restated(s, tier, at_commit)["row"]


def cut_before_stop(case, pair, tier, at_commit=False):
    """Two calls: everything one row before the row where the exceeding stream stops, then the rest."""
    row = stop_row(case, pair.exceed, tier, at_commit)
    assert row is not None and stop_row(case, pair.fit, tier, at_commit) is None
    return [capped(case, row), lengths_of(case).copy()]


def three_cuts(case, tier):
    """The HBM-only cases: row 1, the row before the failing (or last) row, the end."""
    rows = [stop_row(case, s, tier) for s in range(case.S)]
    row = min([r for r in rows if r is not None] + [longest(case) - 1])
    return [capped(case, 1), capped(case, max(row, 1)), lengths_of(case).copy()]


# ------------------------------------------------------------------ the driver
def same(name, got, want, what):
    for field in NAMES:
        a, b = getattr(got, field), want[field] if isinstance(want, dict) else getattr(want, field)
        assert np.array_equal(a, b), "%s: %s of %s differs at word %d" % (what, field, name,
                                                                         int(np.flatnonzero(a != b)[0]))


def sessions_of(case, tier, at_commit=False, device=False, fill=FILL):
    """The host twin's session (and with `device` the device's), everything the byte `fill`."""
    planes = case.packed()[0]
    return [fpred.PredSession(case.S, planes.steps, case.n, planes.dmax, tier, at_commit, fill=fill, host=h)
            for h in ([True, False] if device else [True])]


def drive(case, calls, tier, at_commit=False, device=False, every=True, before_launch=None, fill=FILL,
          executed=False):
    """Feeds the host twin (and with `device` the device) the case's streams call by call, every buffer and the
    state starting as 0xA5 bytes.  After every call (every=False: after the last) the twin equals the
    expectation, and the device the twin, in every word.  executed: committed_and_executed() of every session
    is checked after every call against the same over pred_ref.  Returns the sessions."""
    sessions = sessions_of(case, tier, at_commit, device, fill)
    b = batch(case)
    exp = Expect(case, tier, at_commit)
    seen = [(0, 0)] * case.S
    for i, lens in enumerate(calls):
        for ses in sessions:
            ses.launch(*b, lens, before_launch=before_launch)
        want = exp.after(lens)
        if every or i == len(calls) - 1:
            what = "%s at %s, call %d of %d" % (case.name, R.TIER_NAME[tier], i, len(calls))
            host = sessions[0].result()
            same("the host twin", host, want, what)
            results = [host]
            if device:
                results.append(sessions[1].result())
                same("the device", results[1], host, what)
            if executed:
                # mod.rs:92-97 over pred_ref: the rows handed over since the last look, the dots its order gained
                ref = []
                for s, st in enumerate(case.streams):
                    order = exp.g[s].order
                    ref.append((exp.done[s] - seen[s][0], [tuple(st[r][0]) for r in order[seen[s][1]:]]))
                    seen[s] = (exp.done[s], len(order))
                for ses, res in zip(sessions, results):
                    assert ses.committed_and_executed(lens, res) == ref, what
    return sessions


# ------------------------------------------------------------------ hand-built streams across a cut
NEVER = E.NEVER
# (rows, the stream's lengths in the first, second and third call)
BASE = [((1, 1), [(2, 1)], (1, 1)), ((1, 2), [(1, 1)], (2, 1)), ((3, 1), [(1, 2)], (3, 3)), ((2, 1), [], (4, 2))]
# the closer (2, 1) has the lowest clock: released from phase one, (1, 1) waits for it in phase two
LOW = [((1, 1), [(2, 1)], (2, 1)), ((1, 2), [(1, 1)], (3, 1)), ((3, 1), [(1, 2)], (4, 3)), ((2, 1), [], (1, 2))]
# seqs 3, 5, 2 of source 1 commit and execute before seq 1: both windows hold bits above the frontier at the
# cut; (2, 1) waits on seq 1 (phase one) and seq 4, (3, 1) then finds 3 and 5 executed by ring bit and by frontier
ABOVE = [((1, 3), [], (3, 1)), ((1, 5), [], (5, 1)), ((1, 2), [], (2, 1)), ((2, 1), [(1, 1), (1, 4), (1, 5)], (9, 2)),
         ((1, 1), [], (1, 1)), ((3, 1), [(1, 3), (1, 5), (1, 2)], (10, 3)), ((1, 4), [(2, 1)], (4, 1))]
HAND = [
    (BASE, (3, 4, 4)),                                                    # the cut after row 2
    (BASE, (1, 4, 4)),                                                    # after row 0
    (BASE, (2, 3, 4)),                                                    # after row 1, and again after row 2
    (LOW, (3, 4, 4)),
    (LOW, (2, 3, 4)),
    (ABOVE, (4, 5, 7)),
    (ABOVE, (3, 6, 7)),
    (BASE[:3] + [((1, 2), [], (9, 1))] + BASE[3:], (3, 5, 5)),            # a repeat of a dot pending since call 0
    ([((1, 1), [], (1, 1)), ((2, 1), [NEVER], (2, 2)), ((1, 1), [], (3, 1)), ((3, 1), [], (4, 3))], (2, 3, 4)),
    #                                                                       ... of one that executed in call 0
    (BASE[:2] + [((0, 1), [], (7, 1))] + BASE[2:], (2, 4, 5)),             # source 0 in a later call
    (BASE, (0, 0, 4)),                                                    # untouched by two calls, then whole
    (LOW, (0, 4, 4)),
]
HAND_ERR = [0] * 7 + [R.FX_ERR_DOUBLE_INDEX] * 2 + [R.FX_ERR_DOT_RANGE] + [0] * 2
HAND_NEXEC = [4, 4, 4, 4, 4, 7, 7, 0, 1, 0, 4, 4]


def hand_case(compiled=False):
    """The hand-built streams at n = 3 (the generic layouts) or as n = 5, dmax = 5 (the compiled SMALL layout)."""
    streams = [E.T(rows) for rows, _ in HAND]
    if compiled:
        return E.Case("hand-built compiled", 5, streams, [SMALL], 5)
    return E.Case("hand-built", 3, streams, [SMALL, LDS, HBM])


def hand_calls():
    return [np.array([cuts[c] for _, cuts in HAND], np.uint32) for c in range(3)]


def check_hand_streams_hold_registrations():
    """From pred_ref.Graph: after row 2 of the base stream nothing has executed and both phase indexes hold
    registrations; row 3 executes all four at step 3.  With the low-clock closer the same, (2, 1) first."""
    for rows, first in ((BASE, 0), (LOW, 3)):
        g = R.Graph(3)
        for rec, (dot, deps, clock) in enumerate(rows):
            if rec == 3:
                assert g.order == [] and g.nreg[0] > 0 and g.nreg[1] > 0
            g.step = rec
            g.add(dot, rec, clock, set(deps))
        assert sorted(g.order) == [0, 1, 2, 3] and g.order[0] == first
        assert all(g.release[r] == 3 for r in range(4)) and g.nreg == [0, 0]
    g = R.Graph(3)
    for rec, (dot, deps, clock) in enumerate(ABOVE[:4]):
        g.step = rec
        g.add(dot, rec, clock, set(deps))
    for clock in (g.committed_clock, g.executed_clock):
        assert clock.front[1] == 0 and clock.above[1] == {2, 3, 5}
    assert g.nreg[0] == 2
