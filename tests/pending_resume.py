"""Sessions of the pending stage (fx_pending_advance): what every call must
leave, and the driver that feeds sessions call by call and compares them.  The
partitions are kv_resume's.  Shared by the CPU and the GPU tests.

What a call must leave is stated against the whole stage: the words of
fx_pending_aggregate_host at the HBM tier over this call's nexec, on buffers of
0xA5 bytes.  A failing stream stops at the same row on both, so it needs no
special case; `Model` restates the two refusals that hold for one call alone
(nexec > steps behind FX_FLAG_INIT's call, nexec < done)."""
import numpy as np

from fantoch_amd import _lib
from fantoch_amd import pending as P

from kv_resume import A5, FILL, INVALID, OVERFLOW, capped, cut_pairs, cuts_of_64, one_call, row_per_call  # noqa: F401


class Model:
    def __init__(self, case):
        self.case = case
        self.eff = np.zeros(case.S, np.uint32)    # the nexec whose whole run the outputs equal
        self.done = np.zeros(case.S, np.uint32)
        self.status = np.zeros(case.S, np.uint32)
        self.over = np.zeros(case.S, np.uint32)   # the status of the last call where it is the call's alone
        self.mask = np.zeros(case.S, bool)

    def whole(self, nexec):
        c = self.case
        return P.run_pending_host(c.order, nexec, c.rifl, c.count, c.S, c.steps, c.count_mask, c.process, P.HBM,
                                  fill=FILL)

    def call(self, nexec, init):
        nexec = np.asarray(nexec, np.uint32)
        if init:
            self.eff[:] = self.done[:] = self.status[:] = 0
        self.over[:] = 0
        self.mask = np.zeros(self.case.S, bool)
        probe = self.whole(np.minimum(nexec, self.case.steps))
        for s, n in enumerate(int(x) for x in nexec):
            done = int(self.done[s])
            if self.status[s]:
                continue
            if n > self.case.steps:
                if init:
                    self.eff[s] = n  # the whole stage's refusal, word for word
                else:
                    self.over[s], self.mask[s] = OVERFLOW, True
            elif not init and n <= done:
                self.over[s], self.mask[s] = INVALID if n < done else 0, True
            else:
                self.eff[s] = self.done[s] = n
                self.status[s] = probe.err[s]

    def expected(self):
        want = self.whole(self.eff)
        err = want.err.copy()
        err[self.mask] = self.over[self.mask]
        return dict({name: getattr(want, name) for name in P.NAMES}, err=err)


def same(name, got, want, what, fields=P.NAMES):
    for field in fields:
        a, b = getattr(got, field), want[field] if isinstance(want, dict) else getattr(want, field)
        assert np.array_equal(a, b), "%s: %s of %s differs at word %d" % (what, field, name,
                                                                         int(np.flatnonzero(a != b)[0]))


def drive(case, calls, device=False, every=True, before_launch=None, sessions=None, model=None, init_first=True):
    """Feeds the host twin (and with `device` the device) the case's planes call
    by call, every buffer and the state starting as 0xA5 bytes.  After every
    call (every=False: after the last) the twin equals Model.expected and the
    device the twin, in every output word.  Returns (sessions, model)."""
    if sessions is None:
        sessions = [P.PendingSession(case.S, case.steps, case.count_mask, case.process, fill=FILL, host=True)]
        if device:
            sessions.append(P.PendingSession(case.S, case.steps, case.count_mask, case.process, fill=FILL))
        model = Model(case)
    for i, nexec in enumerate(calls):
        init = init_first and i == 0
        for ses in sessions:
            ses.launch(case.order, nexec, case.rifl, case.count, init=init, before_launch=before_launch)
        model.call(nexec, init)
        if every or i == len(calls) - 1:
            what = "%s, call %d of %d" % (case.name, i, len(calls))
            host = sessions[0].result()
            same("the host twin", host, model.expected(), what)
            for ses in sessions[1:]:
                same("the device", ses.result(), host, what)
    return sessions, model
