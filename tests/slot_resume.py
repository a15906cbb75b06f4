"""Sessions of the slot executor (fx_slot_advance): the partitions of a case's
streams into calls, what every call must leave (one whole run over the rows
handed over so far, fill included), and the driver that feeds sessions call by
call and compares them.  Shared by the CPU and the GPU tests."""
import numpy as np

from fantoch_amd import slot as fslot

import slot_shapes as SS

_EXPECTED = {}


def expected_after(case, lens, at_commit=False):
    """order, release, nexec, err after the call that brought the streams to `lens`
    rows: those of one whole run over buffers of 0xA5 bytes (computed once per
    (case, lens, mode) and shared: treat as read-only)."""
    lens = [min(int(l), len(st)) for st, l in zip(case.streams, lens)]
    key = (case.name, case.S, tuple(lens), at_commit)
    if key not in _EXPECTED:
        _EXPECTED[key] = SS.Case(case.name, [st[:l] for st, l in zip(case.streams, lens)],
                                 case.steps).expected(SS.SCAN, at_commit)
    return _EXPECTED[key]


# ------------------------------------------------------------------ partitions: a list of lengths per call
def capped(case, cut):
    return np.minimum(case.lengths, np.uint32(cut)).astype(np.uint32)


def one_call(case):
    return [case.lengths.copy()]


def row_per_call(case):
    return [capped(case, c) for c in range(1, max(int(case.lengths.max(initial=0)), 1) + 1)]


def cuts_of_64(case):
    """A call at every multiple of 64 rows, then the rest."""
    return [capped(case, c) for c in range(64, case.steps, 64)] + [case.lengths.copy()]


def cut_pairs(case, seed):
    """Three calls; stream s is cut at its own two rows 0 <= c1 <= c2 <= L, so a
    call moves different streams by different amounts.  Every fifth stream has
    c1 == c2 (its second call is empty), every seventh c1 == 0, every eleventh
    c2 == L (its last call is empty)."""
    rng = np.random.default_rng(seed)
    L = case.lengths.astype(np.int64)
    c = np.sort(np.stack([rng.integers(0, L + 1), rng.integers(0, L + 1)]), axis=0)
    s = np.arange(case.S)
    c[0] = np.where(s % 7 == 3, 0, c[0])
    c[1] = np.where(s % 11 == 5, L, c[1])
    c[0] = np.where(s % 5 == 1, c[1], c[0])
    return [c[0].astype(np.uint32), c[1].astype(np.uint32), case.lengths.copy()]


# ------------------------------------------------------------------ the driver
def same(name, got, want, what):
    for field in fslot.NAMES:
        a, b = getattr(got, field), want[field] if isinstance(want, dict) else getattr(want, field)
        assert np.array_equal(a, b), "%s: %s of %s differs at word %d" % (what, field, name,
                                                                         int(np.flatnonzero(a != b)[0]))


def drive(case, calls, at_commit=False, device=False, every=True, before_launch=None, fill=SS.FILL):
    """Feeds the host twin (and with `device` the device) the case's streams call
    by call, every buffer and the state starting as 0xA5 bytes.  After every
    call (every=False: after the last) the twin equals expected_after, and the
    device the twin, in every word.  Returns the sessions."""
    sessions = [fslot.SlotSession(case.S, case.steps, at_commit, fill=fill, host=True)]
    if device:
        sessions.append(fslot.SlotSession(case.S, case.steps, at_commit, fill=fill, host=False))
    for i, lens in enumerate(calls):
        for ses in sessions:
            ses.launch(case.plane, lens, before_launch=before_launch)
        if every or i == len(calls) - 1:
            what = "%s, call %d of %d" % (case.name, i, len(calls))
            host = sessions[0].result()
            same("the host twin", host, expected_after(case, lens, at_commit), what)
            if device:
                same("the device", sessions[1].result(), host, what)
    return sessions
