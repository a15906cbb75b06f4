"""Sessions of the KV stage on the host twin (fx_kv_advance_host,
fx_kv_session_monitor_host): after every call of every partition the outputs
equal one fx_kv_execute_host over the rows accepted so far (kv_resume.Model),
and for a sample the restatement kv_ref.  Every buffer, the state included,
starts as 0xA5 bytes.  No GPU needed."""
import ctypes
import random

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import kv as K

import kv_ref
import kv_resume as R
import kv_shapes as KS

CASES = KS.all_cases()
IDS = [c.name for c in CASES]
INVALID, OVERFLOW = _lib.FX_ERR_INVALID_ARG, _lib.FX_ERR_ORDER_OVERFLOW
A5 = R.A5


def case_named(name):
    return [c for c in CASES if c.name == name][0]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_one_call_equals_the_whole_stage(i):
    case = CASES[i]
    sessions, model = R.drive(case, R.one_call(case), monitor=True)
    res, mon, whole = sessions[0].result(), sessions[0].monitor(fill=R.FILL), case.run_host()
    for s, st in enumerate(case.streams):
        if st.get("err") == INVALID:  # the whole stage writes err alone; the session keeps the empty prefix
            assert int(res.err[s]) == INVALID and np.all(res.store[s] == A5) and np.all(mon.mon_off[s] == 0)
        else:
            assert int(res.err[s]) == int(whole.err[s])
            if not st.get("err"):
                assert np.array_equal(res.store[s], whole.store[s]) and np.array_equal(mon.mon_off[s], whole.mon_off[s])
    if not any(st.get("err") for st in case.streams):
        R.same("the session", res, whole, case.name, ("result", "store", "err"))
        R.same("the monitor", mon, whole, case.name, R.MONITOR_FIELDS)
        case.check(mon)  # kv_ref, through the shapes' own check


@pytest.mark.parametrize("cuts", ["64", "pairs 1", "pairs 2"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_cut_streams_after_every_call(i, cuts):
    case = CASES[i]
    calls = R.cuts_of_64(case) if cuts == "64" else R.cut_pairs(case, int(cuts[-1]))
    R.drive(case, calls, monitor=(cuts != "pairs 2"))


@pytest.mark.parametrize("name", ["patterns k64", "slots o4 k64", "errors k600", "monitor k600"])
def test_one_row_per_call(name):
    case = case_named(name)
    R.drive(case, R.row_per_call(case), monitor=name.startswith("monitor"))


def test_pieces_against_the_restatement():
    """kv_ref over the rows consumed so far, after every call of a cut pair."""
    case = case_named("patterns k64")
    calls = R.cut_pairs(case, 3)
    ses = K.KvSession(case.S, case.steps, case.keys, case.omax, fill=R.FILL, host=True)
    for nexec in calls:
        ses.launch(case.order, nexec, case.key, case.ops, case.key_mask)
        mon = ses.monitor(fill=R.FILL)
        for s, st in enumerate(case.streams):
            kv_ref.check_stream(mon, s, st["order"][:int(nexec[s])], st["keys_of"], st["ops_of"])


# ------------------------------------------------------------------ contract edges
def states(sessions):
    return [ses.state_words() for ses in sessions]


def advance(sessions, case, nexec, **kw):
    res = [ses.advance(case.order, nexec, case.key, case.ops, case.key_mask, **kw) for ses in sessions]
    for r in res[1:]:
        R.same("the device", r, res[0], "advance")
    return res[0]


def unchanged(res, first, but=("err",)):
    for f in K.SESSION_NAMES:
        if f not in but:
            assert np.array_equal(np.ravel(getattr(res, f)), np.ravel(getattr(first, f))), f


def test_a_call_without_new_rows_rewrites_err_alone():
    case = case_named("patterns k64")
    nexec = R.capped(case, 70)
    sessions, _ = R.drive(case, [nexec])
    first, before = sessions[0].result(), states(sessions)
    sessions[0].fill_outputs(0x11, ("err",))
    res = advance(sessions, case, nexec)
    assert np.all(res.err == 0)
    unchanged(res, first)
    assert np.array_equal(states(sessions)[0], before[0])


def test_a_shorter_nexec_is_refused_for_its_stream_and_the_session_continues():
    case = case_named("edges S65 k5")
    nexec = R.cut_pairs(case, 4)[1]
    sessions, model = R.drive(case, [nexec])
    first, before = sessions[0].result(), states(sessions)
    short = nexec.copy()
    shrunk = np.flatnonzero(nexec > 0)[::2]
    short[shrunk] -= 1
    res = advance(sessions, case, short)
    want = np.zeros(case.S, np.uint32)
    want[shrunk] = INVALID
    assert np.array_equal(res.err, want)
    unchanged(res, first)
    assert np.array_equal(states(sessions)[0], before[0])
    model.call(short, False)
    R.drive(case, [case.nexec], sessions=sessions, model=model, init_first=False, monitor=True)


def test_nexec_above_steps_is_refused_for_the_call_and_the_session_continues():
    case = case_named("edges S65 k5")
    nexec = R.capped(case, 40)
    sessions, model = R.drive(case, [nexec])
    first, before = sessions[0].result(), states(sessions)
    over = nexec.copy()
    over[::3] = case.steps + 1
    res = advance(sessions, case, over)
    want = np.zeros(case.S, np.uint32)
    want[::3] = OVERFLOW
    assert np.array_equal(res.err, want)
    unchanged(res, first)
    assert np.array_equal(states(sessions)[0], before[0])
    model.call(over, False)
    R.drive(case, [case.nexec], sessions=sessions, model=model, init_first=False)


@pytest.mark.parametrize("change", [dict(steps=130), dict(steps=132), dict(keys=4), dict(keys=6), dict(omax=2)],
                         ids=str)
def test_a_call_that_breaks_the_session_contract(change):
    """Other steps, keys or omax: FX_ERR_INVALID_ARG for every stream, the state and every other word as they
    were; the session then goes on."""
    case = case_named("edges S65 k5")
    nexec = R.capped(case, 3)
    sessions, model = R.drive(case, [nexec])
    first, before = sessions[0].result(), states(sessions)
    ops = np.concatenate([case.ops, case.ops]) if "omax" in change else case.ops
    res = sessions[0].advance(case.order, case.nexec, case.key, ops, case.key_mask, **change)
    assert np.all(res.err == INVALID)
    unchanged(res, first)
    assert np.array_equal(states(sessions)[0], before[0])
    R.drive(case, [case.nexec], sessions=sessions, model=model, init_first=False)


def test_a_state_that_never_saw_init():
    case = case_named("edges S65 k5")
    ses = K.KvSession(case.S, case.steps, case.keys, case.omax, fill=R.FILL, host=True)
    before = ses.state_words()
    res = ses.advance(case.order, case.nexec, case.key, case.ops, case.key_mask, init=False)
    assert np.all(res.err == INVALID)
    assert np.all(res.result == A5) and np.all(res.store == A5) and np.all(res.rank == A5)
    assert np.array_equal(ses.state_words(), before)
    mon = ses.monitor(fill=R.FILL)
    assert np.all(mon.err == INVALID) and np.all(mon.mon_off == A5) and np.all(mon.monitor == A5)


def test_init_on_a_used_state_equals_a_fresh_session():
    used, rng = KS.chunk_edges(65, 5), random.Random(9)
    other = KS.Case("other", [KS.rand_stream(rng, 131, 50 + s % 60, 5, 1) for s in range(65)], 5, 1)
    sessions, _ = R.drive(used, R.cuts_of_64(used)[:2])
    sessions[0].fill_outputs(R.FILL)
    fresh, model = R.drive(other, [other.nexec], monitor=True)
    R.drive(other, [other.nexec], sessions=sessions, model=R.Model(other), monitor=True)
    R.same("the used session", sessions[0].result(), fresh[0].result(), "after FX_FLAG_INIT")
    assert np.array_equal(sessions[0].state_words(), fresh[0].state_words())


def test_refusals_before_any_work():
    case = case_named("edges S1 k5")
    lib = _lib.load()
    ses = K.KvSession(case.S, case.steps, case.keys, case.omax, fill=R.FILL, host=True)
    arrs = [np.ascontiguousarray(x, np.uint32) for x in (case.order, case.nexec, case.key, case.ops)]
    outs = [ses.out[n].ctypes.data for n in K.SESSION_NAMES]

    def call(inb, outb, state, flags):
        return lib.fx_kv_advance_host(ctypes.byref(inb), ctypes.byref(outb), state, flags)

    def batch(**kw):
        f = dict(order=arrs[0].ctypes.data, nexec=arrs[1].ctypes.data, key=arrs[2].ctypes.data, key_mask=0xFFFFFFFF,
                 ops=arrs[3].ctypes.data, num_streams=case.S, steps=case.steps, keys=case.keys, omax=case.omax)
        f.update(kw)
        return _lib.KvBatch(*[f[n] for n, _ in _lib.KvBatch._fields_])

    good, state = _lib.KvSessionOut(*outs), ses.state.ctypes.data
    assert call(batch(), good, None, _lib.FX_FLAG_INIT) == INVALID
    assert call(batch(), good, state, _lib.FX_FLAG_INIT | _lib.FX_FLAG_EXECUTE_AT_COMMIT) == INVALID
    for i in range(4):
        o = list(outs)
        o[i] = None
        assert call(batch(), _lib.KvSessionOut(*o), state, _lib.FX_FLAG_INIT) == INVALID
    for kw in (dict(order=None), dict(nexec=None), dict(key=None), dict(ops=None), dict(omax=0), dict(omax=5),
               dict(keys=0), dict(keys=_lib.FX_TABLE_MAX_KEYS + 1)):
        assert call(batch(**kw), good, state, _lib.FX_FLAG_INIT) == INVALID
    assert np.all(ses.state_words() == A5) and np.all(ses.result().err == A5)
    mon = _lib.KvOut(outs[0], outs[1], outs[2], None, outs[3])
    assert lib.fx_kv_session_monitor_host(ctypes.byref(batch()), outs[2], ctypes.byref(mon), state) == INVALID
    assert lib.fx_kv_session_bytes(5, 3) == 3 * (64 + 2 * 64) * 4
    assert lib.fx_kv_session_bytes(65, 1) == (64 + 2 * 128) * 4
    if lib.fx_device_count() <= 0:
        assert lib.fx_kv_advance(ctypes.byref(batch()), ctypes.byref(good), state, _lib.FX_FLAG_INIT, None) == \
            _lib.FX_ERR_NO_DEVICE
