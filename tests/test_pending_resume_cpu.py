"""Sessions of the pending stage on the host twin (fx_pending_advance_host):
after every call of every partition the outputs equal one
fx_pending_aggregate_host at the HBM tier over the same nexec
(pending_resume.Model), and for a sample the restatement pending_ref.  Every
buffer, the state included, starts as 0xA5 bytes.  No GPU needed."""
import ctypes

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import pending as P

import pending_resume as R
import pending_shapes as PS

CASES = PS.all_cases()
IDS = [c.name for c in CASES]
INVALID, OVERFLOW = _lib.FX_ERR_INVALID_ARG, _lib.FX_ERR_ORDER_OVERFLOW
A5 = R.A5


def case_named(name):
    return [c for c in CASES if c.name == name][0]


def ref_check(case, res):
    """pending_ref, through the shapes' own check.  Not for a stream with nexec > steps behind earlier calls:
    there the session keeps what those calls wrote, and the whole stage writes nothing."""
    if all(st.get("nexec", 0) <= case.steps for st in case.streams):
        case.check(res, P.HBM)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_one_call_equals_the_whole_stage(i):
    case = CASES[i]
    sessions, _ = R.drive(case, R.one_call(case))
    res = sessions[0].result()
    R.same("the session", res, case.run_host(P.HBM), case.name)
    case.check(res, P.HBM)  # pending_ref, through the shapes' own check


@pytest.mark.parametrize("cuts", ["64", "pairs 1", "pairs 2"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_cut_streams_after_every_call(i, cuts):
    case = CASES[i]
    calls = R.cuts_of_64(case) if cuts == "64" else R.cut_pairs(case, int(cuts[-1]))
    sessions, _ = R.drive(case, calls)
    ref_check(case, sessions[0].result())


@pytest.mark.parametrize("name", ["pairs and wide", "rifl reuse", "errors", "process 2", "hbm buckets"])
def test_one_row_per_call(name):
    case = case_named(name)
    sessions, _ = R.drive(case, R.row_per_call(case))
    ref_check(case, sessions[0].result())


def test_new_ready_is_the_window_of_the_last_call():
    case = case_named("pairs and wide")
    ses = P.PendingSession(case.S, case.steps, case.count_mask, case.process, fill=R.FILL, host=True)
    seen = [[] for _ in range(case.S)]
    for nexec in R.cuts_of_64(case) + [case.nexec]:  # the last call brings nothing new
        res = ses.advance(case.order, nexec, case.rifl, case.count)
        for s in range(case.S):
            new = ses.new_ready(s)
            seen[s] += new
            assert seen[s] == res.ready_heads(s)
    assert all(ses.new_ready(s) == [] for s in range(case.S)) and sum(len(x) for x in seen) > 100


# ------------------------------------------------------------------ contract edges
def unchanged(res, first, but=("err",)):
    for f in P.NAMES:
        if f not in but:
            assert np.array_equal(getattr(res, f), getattr(first, f)), f


def advance(ses, case, nexec, **kw):
    return ses.advance(case.order, nexec, case.rifl, case.count, **kw)


def test_a_call_without_new_rows_rewrites_err_alone():
    case = case_named("rifl reuse")
    nexec = R.capped(case, 70)
    (ses,), _ = R.drive(case, [nexec])
    first, before = ses.result(), ses.state_words()
    ses.fill_outputs(0x11, ("err",))
    res = advance(ses, case, nexec)
    assert np.all(res.err == 0)
    unchanged(res, first)
    assert np.array_equal(ses.state_words(), before)


def test_a_shorter_nexec_is_refused_for_its_stream_and_the_session_continues():
    case = case_named("edges S65")
    nexec = R.cut_pairs(case, 4)[1]
    (ses,), model = R.drive(case, [nexec])
    first, before = ses.result(), ses.state_words()
    short = nexec.copy()
    shrunk = np.flatnonzero(nexec > 0)[::2]
    short[shrunk] -= 1
    res = advance(ses, case, short)
    want = np.zeros(case.S, np.uint32)
    want[shrunk] = INVALID
    assert np.array_equal(res.err, want)
    unchanged(res, first)
    assert np.array_equal(ses.state_words(), before)
    model.call(short, False)
    R.drive(case, [case.nexec], sessions=[ses], model=model, init_first=False)


def test_nexec_above_steps_is_refused_for_the_call_and_the_session_continues():
    case = case_named("edges S65")
    nexec = R.capped(case, 40)
    (ses,), model = R.drive(case, [nexec])
    first, before = ses.result(), ses.state_words()
    over = nexec.copy()
    over[::3] = case.steps + 1
    res = advance(ses, case, over)
    want = np.zeros(case.S, np.uint32)
    want[::3] = OVERFLOW
    assert np.array_equal(res.err, want)
    unchanged(res, first)
    assert np.array_equal(ses.state_words(), before)
    model.call(over, False)
    R.drive(case, [case.nexec], sessions=[ses], model=model, init_first=False)


@pytest.mark.parametrize("change", [dict(steps=130), dict(steps=132), dict(count_mask=0xFF), dict(process=1)], ids=str)
def test_a_call_that_breaks_the_session_contract(change):
    """Other steps, count_mask or process: FX_ERR_INVALID_ARG for every stream, the state and every other word
    as they were; the session then goes on."""
    case = case_named("edges S65")
    (ses,), model = R.drive(case, [R.capped(case, 3)])
    first, before = ses.result(), ses.state_words()
    res = advance(ses, case, case.nexec, **change)
    assert np.all(res.err == INVALID)
    unchanged(res, first)
    assert np.array_equal(ses.state_words(), before)
    R.drive(case, [case.nexec], sessions=[ses], model=model, init_first=False)


def test_a_state_that_never_saw_init():
    case = case_named("edges S65")
    ses = P.PendingSession(case.S, case.steps, case.count_mask, case.process, fill=R.FILL, host=True)
    before = ses.state_words()
    res = advance(ses, case, case.nexec, init=False)
    assert np.all(res.err == INVALID)
    assert all(np.all(getattr(res, f) == A5) for f in P.NAMES if f != "err")
    assert np.array_equal(ses.state_words(), before)
    assert ses.new_ready(0) == []


def test_init_on_a_used_state_equals_a_fresh_session():
    used, other = case_named("capacity"), PS.reuse()
    other = PS.Case("other", (other.streams * 2)[:used.S], steps=used.steps)
    (ses,), _ = R.drive(used, R.cuts_of_64(used)[:2])
    ses.fill_outputs(R.FILL)
    (fresh,), _ = R.drive(other, R.cuts_of_64(other))
    R.drive(other, R.cuts_of_64(other), sessions=[ses], model=R.Model(other))
    R.same("the used session", ses.result(), fresh.result(), "after FX_FLAG_INIT")


def test_refusals_before_any_work():
    case = case_named("edges S1")
    lib = _lib.load()
    ses = P.PendingSession(case.S, case.steps, fill=R.FILL, host=True)
    arrs = [np.ascontiguousarray(x, np.uint32) for x in (case.order, case.nexec, case.rifl, case.count)]
    outs = [ses.out[n].ctypes.data for n in P.NAMES]

    def batch(**kw):
        f = dict(order=arrs[0].ctypes.data, nexec=arrs[1].ctypes.data, rifl=arrs[2].ctypes.data,
                 count=arrs[3].ctypes.data, count_mask=0xFFFFFFFF, process=0, num_streams=case.S, steps=case.steps)
        f.update(kw)
        return _lib.PendingBatch(*[f[n] for n, _ in _lib.PendingBatch._fields_])

    def call(inb, outb, state, flags):
        return lib.fx_pending_advance_host(ctypes.byref(inb), ctypes.byref(outb), state, flags)

    good, state = _lib.PendingOut(*outs), ses.state.ctypes.data
    assert call(batch(), good, None, _lib.FX_FLAG_INIT) == INVALID
    assert call(batch(), good, state, _lib.FX_FLAG_INIT | _lib.FX_FLAG_SAVE_STATE) == INVALID
    for i in range(len(outs)):
        o = list(outs)
        o[i] = None
        assert call(batch(), _lib.PendingOut(*o), state, _lib.FX_FLAG_INIT) == INVALID
    for kw in (dict(order=None), dict(nexec=None), dict(rifl=None), dict(count=None), dict(count_mask=0)):
        assert call(batch(**kw), good, state, _lib.FX_FLAG_INIT) == INVALID
    assert np.all(ses.state_words() == A5) and np.all(ses.result().err == A5)
    assert lib.fx_pending_session_bytes(63, 3) == 3 * (64 * 4 + 64 * 16)
    assert lib.fx_pending_session_bytes(65, 1) == 64 * 4 + 2 * 64 * 16
    if lib.fx_device_count() <= 0:
        assert lib.fx_pending_advance(ctypes.byref(batch()), ctypes.byref(good), state, _lib.FX_FLAG_INIT, None) == \
            _lib.FX_ERR_NO_DEVICE
