"""Sessions of the predecessors executor on the host (fx_pred_advance_host):
for every partition of a case's streams into calls, every output word after
every call is what pred_ref leaves over the rows handed over so far at the
tier's limits (pred_resume.Expect, fill included).  The contract edges and the
refusals of the entry points.  No GPU."""
import ctypes

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import pred as fpred

import pred_edges as E
import pred_ref as PRF
import pred_resume as R

SMALL, LDS, HBM = R.SMALL, R.LDS, R.HBM
CASES = E.all_cases()
RUNS = [(c, t) for c in CASES for t in c.tiers]
RUN_IDS = ["%s at %s" % (c.name, PRF.TIER_NAME[t]) for c, t in RUNS]
ON_CHIP = [(c, t) for c, t in RUNS if t != HBM]
ON_CHIP_IDS = ["%s at %s" % (c.name, PRF.TIER_NAME[t]) for c, t in ON_CHIP]
HBM_ONLY = [c for c in CASES if c.tiers == (HBM,) and c.name in ("vertices HBM", "window HBM")]
PAIRS = [(c, p) for c in CASES for p in c.pairs]
PAIR_IDS = ["%s: %s" % (c.name, p.resource) for c, p in PAIRS]
MODES = pytest.mark.parametrize("at_commit", [False, True], ids=["", "at commit"])
DEVICE = False


def named(name):
    return [c for c in CASES if c.name == name][0]


def one_row_cases():
    return [named("lengths"), named("lengths compiled"), named("errors"), named("errors compiled"),
            E.Case("mixed 40", 3, [E.mixed(s, 40, 3, 4) for s in (1, 2, 3)], [SMALL, LDS, HBM]),
            E.Case("mixed 40 compiled", 5, [E.mixed(s, 40, 5, 5) for s in (4, 5, 6)], [SMALL], 5)]


ONE_ROW = [(c, t) for c in one_row_cases() for t in c.tiers]
ONE_ROW_IDS = ["%s at %s" % (c.name, PRF.TIER_NAME[t]) for c, t in ONE_ROW]


def states(sessions):
    return [ses.state_words() for ses in sessions]


def same_states(sessions, before):
    return all(np.array_equal(a, b) for a, b in zip(states(sessions), before))


def both(sessions, case, lens, **kw):
    """One call on each session; the results (the host's first), all equal in every word."""
    res = [ses.advance(*R.batch(case), lens, **kw) for ses in sessions]
    for r in res[1:]:
        R.same("the device", r, res[0], "lengths %s" % (None if lens is None else list(lens[:8])))
    return res[0]


# ------------------------------------------------------------------ whole runs and cuts
@MODES
@pytest.mark.parametrize("case,tier", RUNS, ids=RUN_IDS)
def test_one_call_equals_the_whole_run(case, tier, at_commit):
    ses = R.drive(case, R.one_call(case), tier, at_commit, device=DEVICE)
    R.same("the host twin", ses[0].result(), case.expected(tier, at_commit), case.name)


@pytest.mark.parametrize("case,tier", ON_CHIP, ids=ON_CHIP_IDS)
def test_cut_after_every_4_rows(case, tier):
    R.drive(case, R.cuts_of(case, 4), tier, device=DEVICE)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("case,tier", ON_CHIP, ids=ON_CHIP_IDS)
def test_cut_pairs_per_stream(case, tier, seed):
    calls = R.cut_pairs(case, seed)
    if case.S >= 60:  # the partition has what it is for: empty calls, and streams that move by different amounts
        L = R.lengths_of(case)
        assert np.any(calls[0] == calls[1]) and np.any(calls[0] == 0) and np.any(calls[1] >= np.minimum(L, 1))
        assert len(set((calls[1].astype(int) - calls[0].astype(int)).tolist())) > 2
    R.drive(case, calls, tier, device=DEVICE)


@pytest.mark.parametrize("case", HBM_ONLY, ids=[c.name for c in HBM_ONLY])
def test_hbm_only_cases_cut_at_three_places(case):
    assert len(HBM_ONLY) == 2
    R.drive(case, R.three_cuts(case, HBM), HBM, device=DEVICE)


@pytest.mark.parametrize("case,pair", PAIRS, ids=PAIR_IDS)
def test_reachable_limits_one_row_before_the_stop(case, pair):
    """The cut lies one row before the row where the exceeding stream stops: it stops in the later call with the
    same err, nexec and fill behind it as whole; the fitting stream fits.  Two further calls with larger lengths
    rewrite nexec and err (clobbered first) and change nothing else, the state included."""
    tier = pair.tier
    calls = R.cut_before_stop(case, pair, tier)
    sessions = R.drive(case, calls, tier, device=DEVICE)
    last = sessions[0].result()
    assert int(last.err[pair.exceed]) == PRF.FX_ERR_CAPACITY and int(last.err[pair.fit]) == 0
    R.same("the host twin", last, case.expected(tier), "the whole run")
    before = states(sessions)
    for extra in (1, 50):
        lens = calls[-1].copy()
        lens[pair.exceed] += extra
        for ses in sessions:
            ses.fill_outputs(0x11, ("nexec", "err"))
        R.same("the host twin", both(sessions, case, lens), last, "a stopped stream, %d rows more" % extra)
    assert same_states(sessions, before)


@pytest.mark.parametrize("case,tier", ONE_ROW, ids=ONE_ROW_IDS)
def test_one_row_per_call_and_committed_and_executed(case, tier):
    """Every residue of done mod 4 occurs and every call has fewer rows than a tile;
    committed_and_executed() after every call against the same over pred_ref."""
    calls = R.row_per_call(case)
    assert len(calls) == R.longest(case)
    R.drive(case, calls, tier, device=DEVICE, executed=True)


@pytest.mark.parametrize("name", ["deps count", "deps header"])
def test_deps_beyond_the_tile_row_cut_after_every_row(name):
    case = named(name)
    for tier in case.tiers:
        R.drive(case, R.row_per_call(case), tier, device=DEVICE)


# ------------------------------------------------------------------ hand-built streams across a cut
@pytest.mark.parametrize("compiled,tier", [(False, SMALL), (False, LDS), (False, HBM), (True, SMALL)],
                         ids=["SMALL", "LDS", "HBM", "compiled"])
def test_hand_built_streams_across_a_cut(compiled, tier):
    R.check_hand_streams_hold_registrations()
    case = R.hand_case(compiled)
    sessions = R.drive(case, R.hand_calls(), tier, device=DEVICE)
    last = sessions[0].result()
    assert [int(x) for x in last.err] == R.HAND_ERR
    assert [int(x) for x in last.nexec] == R.HAND_NEXEC
    for s in (0, 1, 2, 3, 4, 10, 11):  # all four execute at step 3
        assert [int(last.release[_lib.index(a, s, case.packed()[0].steps)]) for a in range(4)] == [3] * 4


# ------------------------------------------------------------------ contract edges
def started(case, tier, lens, at_commit=False):
    sessions = R.drive(case, [lens], tier, at_commit, device=DEVICE)
    return sessions, sessions[0].result(), states(sessions)


def continues(sessions, case, tier, at_commit=False):
    lens = R.lengths_of(case)
    R.same("the host twin", both(sessions, case, lens), R.expected_after(case, lens, tier, at_commit),
           "the proper call behind it")


def test_a_call_without_new_rows_rewrites_nexec_and_err():
    case, tier = named("lengths"), SMALL
    lens = R.capped(case, 5)
    sessions, first, before = started(case, tier, lens)
    for ses in sessions:
        ses.fill_outputs(0x11, ("nexec", "err"))
    R.same("the host twin", both(sessions, case, lens), first, "len == done")
    assert same_states(sessions, before)
    continues(sessions, case, tier)


def test_a_shorter_length_is_refused_for_its_stream_and_the_session_continues():
    case, tier = named("lengths compiled"), SMALL
    lens = R.capped(case, 5)
    sessions, first, before = started(case, tier, lens)
    short = lens.copy()
    shrunk = np.flatnonzero(lens > 0)[::2]
    short[shrunk] -= 1
    host = both(sessions, case, short)
    want_err = first.err.copy()
    want_err[shrunk] = R.INVALID
    assert np.array_equal(host.err, want_err) and np.array_equal(host.nexec, first.nexec)
    assert np.array_equal(host.order, first.order) and np.array_equal(host.release, first.release)
    assert same_states(sessions, before)
    continues(sessions, case, tier)


def contract_changes(case, tier):
    planes = case.packed()[0]
    other = LDS if tier == SMALL else SMALL
    return [dict(steps=planes.steps - 1), dict(steps=planes.steps + 1), dict(execute_at_commit=True),
            dict(tier=other), dict(dmax=planes.dmax + 1), dict(drop_ndeps=True)]


@pytest.mark.parametrize("which", range(6), ids=["steps - 1", "steps + 1", "commit flag", "tier", "dmax + 1", "no ndeps"])
@pytest.mark.parametrize("name,tier", [("lengths", SMALL), ("lengths compiled", SMALL), ("errors", LDS)])
def test_a_call_that_breaks_the_session_contract(name, tier, which):
    """FX_ERR_INVALID_ARG for every stream, the state and every other word as they were; the session goes on.
    (With dmax + 1 the deps planes are read no further than before: the stream is refused from its header.)"""
    case = named(name)
    change = contract_changes(case, tier)[which]
    lens = R.capped(case, 3)
    sessions, first, before = started(case, tier, lens)
    host = both(sessions, case, R.lengths_of(case), **change)
    assert np.all(host.err == R.INVALID) and np.array_equal(host.nexec, first.nexec)
    assert np.array_equal(host.order, first.order) and np.array_equal(host.release, first.release)
    assert same_states(sessions, before)
    continues(sessions, case, tier)


@MODES
@pytest.mark.parametrize("tier", [SMALL, LDS, HBM], ids=["SMALL", "LDS", "HBM"])
def test_a_state_that_never_saw_init(tier, at_commit):
    case = named("lengths")
    sessions = R.sessions_of(case, tier, at_commit, DEVICE)
    before = states(sessions)
    assert all(np.all(w == R.A5) for w in before)
    host = both(sessions, case, R.lengths_of(case), init=False)
    assert np.all(host.err == R.INVALID) and np.all(host.nexec == R.A5)
    assert np.all(host.order == R.A5) and np.all(host.release == R.A5)
    assert same_states(sessions, before)


def corrupt(ses, word, value):
    w = ses.state_words()
    w[word::16][:ses.S] = value
    if ses.host:
        ses.state[:ses.state_bytes] = w.view(np.uint8)
    else:
        ses.state.upload(w)


@pytest.mark.parametrize("word,value", [(6, 1 << 20), (8, 1000), (9, 65)], ids=["done > steps", "nexec > done", "nfree > P"])
def test_a_header_with_a_count_out_of_range_is_refused(word, value):
    """Header words 6, 8, 9 = done, nexec, nfree (fx_pred.h): none of them may index anything."""
    case, tier = named("lengths"), SMALL
    sessions, first, _ = started(case, tier, R.capped(case, 3))
    for ses in sessions:
        corrupt(ses, word, value)
    before = states(sessions)
    host = both(sessions, case, R.lengths_of(case))
    assert np.all(host.err == R.INVALID) and np.array_equal(host.nexec, first.nexec)
    assert np.array_equal(host.order, first.order) and np.array_equal(host.release, first.release)
    assert same_states(sessions, before)


def test_init_on_a_used_state_equals_a_fresh_session():
    used = named("lengths")
    other = E.Case("other", used.n, used.streams[::-1], used.tiers)
    assert other.packed()[0].steps == used.packed()[0].steps and other.dmax == used.dmax
    sessions = R.drive(used, R.cuts_of(used, 4)[:2], SMALL, device=DEVICE)
    for ses in sessions:
        ses.fill_outputs(R.FILL)
    for c in (4, 9):
        lens = R.capped(other, c)
        R.same("the host twin", both(sessions, other, lens, init=(c == 4)), R.expected_after(other, lens, SMALL),
               "after FX_FLAG_INIT")


# ------------------------------------------------------------------ the entry points
class Call:
    """One small batch with every pointer valid, for the refusals."""

    def __init__(self):
        case = named("errors")
        self.planes, self.clo, self.chi, self.nd = case.packed()
        p = self.planes
        self.out = [np.full(k, R.A5, np.uint32) for k in (p.plane, p.plane, p.S, p.S)]
        self.state = np.full(_lib.load().fx_pred_session_bytes(SMALL, p.n, p.dmax, p.S), R.FILL, np.uint8)
        self.lengths = np.asarray(p.lengths, np.uint32)
        base = _lib.StreamBatch(p.dot.ctypes.data, p.hdr.ctypes.data, p.deps.ctypes.data, self.lengths.ctypes.data,
                                p.S, p.steps, p.dmax, p.n)
        self.inb = _lib.PredBatch(base, self.clo.ctypes.data, self.chi.ctypes.data, self.nd.ctypes.data)
        self.outb = _lib.OrderBatch(*[a.ctypes.data for a in self.out])

    def host(self, flags=_lib.FX_FLAG_INIT, inb=True, outb=True, state=True, tier=SMALL):
        return _lib.load().fx_pred_advance_host(ctypes.byref(self.inb) if inb else None,
                                                ctypes.byref(self.outb) if outb else None, tier,
                                                self.state.ctypes.data if state else None, flags)

    def device(self, flags=_lib.FX_FLAG_INIT, inb=True, outb=True, state=True, tier=SMALL):
        return _lib.load().fx_pred_advance(ctypes.byref(self.inb) if inb else None,
                                           ctypes.byref(self.outb) if outb else None, tier,
                                           self.state.ctypes.data if state else None, flags, None)

    def untouched(self):
        return all(np.all(a == R.A5) for a in self.out) and bool(np.all(self.state == R.FILL))


BAD_FLAGS = [_lib.FX_FLAG_SAVE_STATE, 8, _lib.FX_FLAG_INIT | _lib.first_tier_flag(1), 1 << 31]


@pytest.mark.parametrize("side", ["host", "device"])
def test_refusals_come_before_any_store_or_launch(side):
    """FX_ERR_INVALID_ARG for a null in, out, state or plane pointer, what fx_pred_execute refuses (n, dmax, steps,
    no ndeps plane with dmax > 31), a tier above HBM and any flag other than INIT and EXECUTE_AT_COMMIT: on the
    device entry point too, before it looks for a device."""
    c = Call()
    call = getattr(c, side)
    bad = _lib.FX_ERR_INVALID_ARG
    assert call(inb=False) == call(outb=False) == call(state=False) == call(tier=3) == bad
    for flags in BAD_FLAGS:
        assert call(flags=flags) == bad
    for field in ("order", "release", "nexec", "err"):
        keep = getattr(c.outb, field)
        setattr(c.outb, field, None)
        assert call() == bad
        setattr(c.outb, field, keep)
    for field in ("clock_lo", "clock_hi"):
        keep = getattr(c.inb, field)
        setattr(c.inb, field, None)
        assert call() == bad
        setattr(c.inb, field, keep)
    for field in ("dot", "hdr", "deps"):
        keep = getattr(c.inb.base, field)
        setattr(c.inb.base, field, None)
        assert call() == bad
        setattr(c.inb.base, field, keep)
    for field, value in (("n", 0), ("n", 9), ("dmax", 257), ("steps", 1 << 26)):
        keep = getattr(c.inb.base, field)
        setattr(c.inb.base, field, value)
        assert call() == bad
        setattr(c.inb.base, field, keep)
    c.inb.ndeps, c.inb.base.dmax = None, 32
    assert call() == bad
    assert c.untouched()


def test_no_device_is_an_error_not_a_fallback(lib):
    """Without a device only: with one this call would launch over host pointers."""
    if lib.fx_device_count() <= 0:
        c = Call()
        assert c.device() == c.device(_lib.FX_FLAG_EXECUTE_AT_COMMIT) == _lib.FX_ERR_NO_DEVICE
        c.inb.base.num_streams = 0  # the device check comes before the empty batch's FX_OK
        assert c.device() == _lib.FX_ERR_NO_DEVICE
        assert c.untouched()


def test_nothing_to_do_is_ok():
    c = Call()
    S = c.inb.base.num_streams
    c.inb.base.num_streams = 0
    assert c.host() == _lib.FX_OK
    c.inb.base.num_streams, c.inb.base.steps = S, 0
    assert c.host() == _lib.FX_OK
    assert c.untouched()


def test_session_bytes_are_zero_exactly_where_a_tier_does_not_fit():
    """fx_pred_session_bytes == 0 (and FX_ERR_UNSUPPORTED) is for a tier whose tables do not fit 160 KiB;
    pred_ref.tier_limits says which: within n <= 8 and dmax <= 256 every tier fits, the widest included."""
    lib = _lib.load()
    for tier in (SMALL, LDS, HBM):
        for n, d in ((1, 0), (5, 5), (8, 31), (8, 256)):
            assert (lib.fx_pred_session_bytes(tier, n, d, 4) > 0) == (PRF.tier_limits(tier, n, d) is not None)
            assert PRF.tier_limits(tier, n, d) is not None


def test_session_bytes_hold_the_headers_and_the_images():
    """The image of the compiled SMALL layout is the 1,152 words below Lay::frames; the generic one follows
    pred_ref.lay_words less its scratch."""
    lib = _lib.load()
    assert lib.fx_pred_session_bytes(SMALL, 5, 5, 1) == (16 + 1152) * 4
    assert lib.fx_pred_session_bytes(SMALL, 5, 5, 7) == 7 * (16 + 1152) * 4
    for tier, n, d in ((SMALL, 3, 4), (LDS, 3, 4), (LDS, 2, 1)):
        lim = PRF.tier_limits(tier, n, d)
        scratch = lim.FD * 4 + lim.LL + lim.P
        words = PRF.lay_words(lim.P, lim.Q, lim.W // 32, n, d, lim.LL) - scratch
        assert lib.fx_pred_session_bytes(tier, n, d, 3) == 3 * (16 + words) * 4
    assert lib.fx_pred_session_bytes(SMALL, 5, 5, 0) == 0 and lib.fx_pred_session_bytes(3, 5, 5, 1) == 0


def test_lengths_null_means_steps_rows_and_run_pred_host_is_a_one_call_session():
    case = named("clocks")
    planes, clo, chi, nd = case.packed()
    want = case.expected(SMALL)
    ses = fpred.PredSession(case.S, planes.steps, case.n, planes.dmax, SMALL, fill=R.FILL, host=True)
    ses.launch(planes, clo, chi, nd, np.ones(case.S, np.uint32))
    R.same("a session", ses.advance(planes, clo, chi, nd, None), want, "lengths NULL")
    R.same("run_pred_host", fpred.run_pred_host(planes, clo, chi, nd, SMALL, fill=R.FILL), want, "whole")
    for s, hand in enumerate(case.hand):
        assert ses.result().executed(s) == hand
