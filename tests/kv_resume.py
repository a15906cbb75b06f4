"""Sessions of the KV stage (fx_kv_advance, fx_kv_session_monitor): the
partitions of a case's order rows into calls, what every call must leave, and
the driver that feeds sessions call by call and compares them.  Shared by the
CPU and the GPU tests; the partitions also serve the pending stage's sessions
(pending_resume.py).

What a call must leave is stated against the whole stage: the words of
fx_kv_execute_host over the rows the session has accepted so far, on buffers of
0xA5 bytes.  The session differs from the whole stage in three documented
places, which `Model` restates per stream: a stream with an invalid row keeps
what its earlier calls wrote and stays stopped; nexec > steps or nexec < done is
refused for that call alone; a stream whose calls all failed has no store row."""
import numpy as np

from fantoch_amd import _lib
from fantoch_amd import kv as K

A5 = 0xA5A5A5A5
FILL = 0xA5
INVALID, OVERFLOW = _lib.FX_ERR_INVALID_ARG, _lib.FX_ERR_ORDER_OVERFLOW


# ------------------------------------------------------------------ partitions: an nexec array per call
def capped(case, cut):
    return np.minimum(case.nexec, np.uint32(cut)).astype(np.uint32)


def one_call(case):
    return [case.nexec.copy()]


def cuts_of_64(case):
    """A call at every multiple of 64 rows, then the rest."""
    return [capped(case, c) for c in range(64, case.steps, 64)] + [case.nexec.copy()]


def row_per_call(case):
    return [capped(case, c) for c in range(1, min(int(case.nexec.max(initial=0)), case.steps))] + [case.nexec.copy()]


def cut_pairs(case, seed):
    """Three calls; stream s is cut at its own two rows 0 <= c1 <= c2 <= L, so a
    call moves different streams by different amounts.  Every fifth stream has
    c1 == c2 (its second call is empty), every seventh c1 == 0, every eleventh
    c2 == L (its last call is empty)."""
    rng = np.random.default_rng(seed)
    L = np.minimum(case.nexec, case.steps).astype(np.int64)
    c = np.sort(np.stack([rng.integers(0, L + 1), rng.integers(0, L + 1)]), axis=0)
    s = np.arange(case.S)
    c[0] = np.where(s % 7 == 3, 0, c[0])
    c[1] = np.where(s % 11 == 5, L, c[1])
    c[0] = np.where(s % 5 == 1, c[1], c[0])
    return [c[0].astype(np.uint32), c[1].astype(np.uint32), case.nexec.copy()]


# ------------------------------------------------------------------ what a session must hold
def first_bad_rows(case):
    """Per stream the first order row fx_kv_execute refuses (the stream's rows if none)."""
    out = []
    for s in range(case.S):
        ne = min(int(case.nexec[s]), case.steps)
        bad = ne
        for k in range(ne):
            a = int(case.order[_lib.index(k, s, case.steps)]) & 0x7FFFFFFF
            ok = a < case.steps
            if ok:
                at = int(_lib.index(a, s, case.steps))
                ok = (int(case.key[at]) & case.key_mask) < case.keys
                ended = False
                for j in range(case.omax):
                    op = int(case.ops[j * case.plane + at])
                    kind = op >> 30
                    if kind == K.EMPTY:
                        ended = True
                    elif ended or (kind == K.PUT and op & K.VALUE_MASK == 0):
                        ok = False
            if not ok:
                bad = k
                break
        out.append(bad)
    return out


class Model:
    """The session's bookkeeping per stream, restated: done, the sticky status, the status of the last call."""

    def __init__(self, case):
        self.case, self.bad = case, first_bad_rows(case)
        self.done = np.zeros(case.S, np.uint32)
        self.status = np.zeros(case.S, np.uint32)
        self.err = np.full(case.S, A5, np.uint32)
        self.stored = np.zeros(case.S, bool)  # some call of the stream went through

    def call(self, nexec, init):
        for s, n in enumerate(int(x) for x in nexec):
            if init:
                self.done[s] = self.status[s] = 0
            done = int(self.done[s])
            if self.status[s]:
                self.err[s] = self.status[s]
            elif n > self.case.steps:
                self.err[s] = OVERFLOW
            elif not init and n <= done:
                self.err[s] = INVALID if n < done else 0
            elif done <= self.bad[s] < n:
                self.err[s] = self.status[s] = INVALID
            else:
                self.done[s], self.err[s], self.stored[s] = n, 0, True

    def whole(self):
        c = self.case
        return K.run_kv_host(c.order, self.done, c.key, c.ops, c.S, c.steps, c.keys, c.omax, c.key_mask, fill=FILL)

    def expected(self):
        """result, store, rank, err after the calls so far, and the whole run they come from."""
        c, whole = self.case, self.whole()
        assert np.all(whole.err == 0)
        store = whole.store.copy()
        store[~self.stored] = A5
        rank = np.full(c.plane, A5, np.uint32)
        for s in range(c.S):
            for k in range(c.keys):
                lo, hi = int(whole.mon_off[s, k]), int(whole.mon_off[s, k + 1])
                if hi > lo:
                    rows = whole.monitor[_lib.index(np.arange(lo, hi), s, c.steps)]
                    rank[_lib.index(rows.astype(np.int64), s, c.steps)] = np.arange(hi - lo, dtype=np.uint32)
        return dict(result=whole.result, store=store, rank=rank, err=self.err.copy()), whole


def same(name, got, want, what, fields=K.SESSION_NAMES):
    for field in fields:
        a = np.asarray(getattr(got, field)).ravel()
        b = np.asarray(want[field] if isinstance(want, dict) else getattr(want, field)).ravel()
        assert np.array_equal(a, b), "%s: %s of %s differs at word %d" % (what, field, name,
                                                                         int(np.flatnonzero(a != b)[0]))


MONITOR_FIELDS = ("monitor", "mon_off", "store", "err")


def check_monitor(sessions, model, whole, what):
    """fx_kv_session_monitor on every side: the whole run's monitor, mon_off and store; err the stream's status."""
    want = dict(monitor=whole.monitor, mon_off=whole.mon_off, store=whole.store, err=model.status)
    mons = [ses.monitor(fill=FILL) for ses in sessions]
    same("the host twin's monitor", mons[0], want, what, MONITOR_FIELDS)
    for m in mons[1:]:
        same("the device's monitor", m, mons[0], what, MONITOR_FIELDS)


def drive(case, calls, device=False, every=True, monitor=False, before_launch=None, sessions=None, model=None,
          init_first=True):
    """Feeds the host twin (and with `device` the device) the case's planes call
    by call, every buffer and the state starting as 0xA5 bytes.  After every
    call (every=False: after the last) the twin equals Model.expected, the
    device the twin in every output word and in every state word, and with
    `monitor` so do the monitors.  Returns (sessions, model)."""
    if sessions is None:
        sessions = [K.KvSession(case.S, case.steps, case.keys, case.omax, fill=FILL, host=True)]
        if device:
            sessions.append(K.KvSession(case.S, case.steps, case.keys, case.omax, fill=FILL, host=False))
        model = Model(case)
    for i, nexec in enumerate(calls):
        init = init_first and i == 0
        for ses in sessions:
            ses.launch(case.order, nexec, case.key, case.ops, case.key_mask, init=init, before_launch=before_launch)
        model.call(nexec, init)
        if every or i == len(calls) - 1:
            what = "%s, call %d of %d" % (case.name, i, len(calls))
            want, whole = model.expected()
            host = sessions[0].result()
            same("the host twin", host, want, what)
            for ses in sessions[1:]:
                same("the device", ses.result(), host, what)
                assert np.array_equal(ses.state_words(), sessions[0].state_words()), what + ": the states differ"
            if monitor:
                check_monitor(sessions, model, whole, what)
    return sessions, model
