"""Sessions of the KV stage on the device (fx_kv_advance,
fx_kv_session_monitor): in every test two sessions, the device's and the host
twin's, fed the same calls and compared byte for byte after every call,
outputs and state; the twin against one whole run over the rows accepted so
far (kv_resume.Model).  Every buffer, the state included, starts as 0xA5 bytes
and the register file is filled with garbage before the launches.  GPU only."""
import random

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import kv as K

import kv_resume as R
import kv_shapes as KS
from kv_shapes import D, G, P
from test_sim_poison import FILLS, poisoner

pytestmark = pytest.mark.gpu

INVALID, OVERFLOW = _lib.FX_ERR_INVALID_ARG, _lib.FX_ERR_ORDER_OVERFLOW
A5 = R.A5
KEYS = [1, 64, 65, _lib.FX_KV_ONCHIP_KEYS, KS.ABOVE]  # 65: two entries per owner lane; 512 / ABOVE: LDS / HBM


def rand_case(S, keys, omax, seed, rows=131):
    rng = random.Random(seed)
    counts = [0, 1, 63, 64, 65, 129, rows]
    return KS.Case("random S%d k%d o%d" % (S, keys, omax),
                   [KS.rand_stream(rng, rows, min(rows, rng.choice(counts)) if s % 3 else rows, keys, omax)
                    for s in range(S)], keys, omax, flag_every=3)


def cuts_63_64_65(case):
    """Stream s cut 63, 64 or 65 rows in, then as many rows again, then the rest."""
    first = np.array([63 + s % 3 for s in range(case.S)], np.uint32)
    return [np.minimum(first, case.nexec), np.minimum(2 * first, case.nexec), case.nexec.copy()]


@pytest.mark.parametrize("omax", [1, 4])
@pytest.mark.parametrize("keys", KEYS)
def test_keys_and_op_slots_cut_63_64_and_65_rows_in(gpu, keys, omax):
    case = rand_case(7, keys, omax, 10 * keys + omax)
    R.drive(case, cuts_63_64_65(case), device=True, monitor=True, before_launch=poisoner(*FILLS[keys % len(FILLS)]))


@pytest.mark.parametrize("keys", [65, KS.ABOVE])
def test_values_and_ranks_carried_from_call_to_call(gpu, keys):
    k1, k2 = keys - 1, keys // 2
    writes = [[P(1 + i)] for i in range(65)]
    sts = [
        # a key written in the first call and read in the third
        (KS.stream(range(130), [k1] + [k2] * 128 + [k1], [[P(77)]] + [[G]] * 128 + [[G]]), (40, 90, 130)),
        # a DELETE as the key's last write before a cut, read behind it
        (KS.stream(range(70), [k1] * 70, [[P(5)]] * 9 + [[D]] + [[G]] * 60), (10, 11, 70)),
        (KS.stream(range(70), [k2] * 70, [[P(5)]] * 63 + [[D]] + [[G], [P(9)], [D], [G], [G], [G]]), (64, 66, 70)),
        # 65 writes on one key split 1 + 64 and 64 + 1: the rank is carried in the count
        (KS.stream(range(65), [k1] * 65, writes), (1, 65, 65)),
        (KS.stream(range(65), [k1] * 65, writes), (64, 65, 65)),
        # the same on two keys of one owner lane (k and k - 64), interleaved
        (KS.stream(range(130), [k1 if i % 2 else k1 - 64 for i in range(130)], [[P(1 + i)] for i in range(130)]),
         (1, 129, 130)),
    ]
    case = KS.Case("carried k%d" % keys, [st for st, _ in sts], keys, 1)
    calls = [np.array([c[i] for _, c in sts], np.uint32) for i in range(3)]
    sessions, _ = R.drive(case, calls, device=True, monitor=True, before_launch=poisoner(*FILLS[0]))
    res = sessions[1].result()
    assert res.results(0, 129) == [77] and res.results(1, 10) == [0] and res.results(2, 64) == [0]
    assert int(res.rank[_lib.index(64, 3, case.steps)]) == 64 and int(res.rank[_lib.index(64, 4, case.steps)]) == 64


# (rows, the row that is made invalid, how, nexec of the three calls)
BAD = [
    (70, 20, "key", (20, 50, 70)),     # the first row of the second call, valid rows behind it
    (70, 35, "put0", (20, 50, 70)),    # a middle row
    (70, 49, "arow", (20, 50, 70)),    # the last row
    (70, 36, "empty", (20, 50, 70)),
    (70, 69, "key", (20, 50, 70)),     # in the last call: two calls stand
    (140, 100, "put0", (63, 129, 140)),  # behind a whole chunk of valid rows of its call
    (70, 0, "key", (20, 50, 70)),      # in the call with FX_FLAG_INIT: an empty store stays behind
]


@pytest.mark.parametrize("keys", [5, KS.ABOVE])
def test_an_invalid_row_in_a_later_call_stops_the_stream_and_keeps_the_prefix(gpu, keys):
    rng = random.Random(keys)
    sts = []
    for rows, bad, how, _ in BAD:
        st = KS.rand_stream(rng, 140, rows, keys, 2)
        a = st["order"][bad]
        if how == "key":
            st["keys_of"][a] = keys
        elif how == "put0":
            st["ops_of"][a] = [G, P(0)]
        elif how == "empty":
            st["ops_of"][a] = [K.kv_op(K.EMPTY), G]
        else:
            st["order"][bad] = 140 + bad
        sts.append(st)
    sts.append(KS.rand_stream(rng, 140, 140, keys, 2))  # a stream that runs, beside them
    case = KS.Case("invalid rows k%d" % keys, sts, keys, 2, steps=140)
    calls = [np.array([c[i] for *_, c in BAD] + [(30, 90, 140)[i]], np.uint32) for i in range(3)]
    model = R.Model(case)
    assert model.bad[:len(BAD)] == [b for _, b, *_ in BAD]
    sessions, model = R.drive(case, calls, device=True, monitor=True, before_launch=poisoner(*FILLS[1]))
    res = sessions[1].result()
    assert [int(x) for x in res.err] == [INVALID] * len(BAD) + [0]
    assert [int(x) for x in model.done] == [20, 20, 20, 20, 50, 63, 0, 140]
    assert np.all(res.store[6] == A5) and np.all(sessions[1].monitor(fill=R.FILL).store[6] == 0)
    # later calls with more rows for the stopped streams: err is rewritten (it is clobbered first), no other word
    before = [ses.state_words() for ses in sessions]
    for ses in sessions:
        ses.fill_outputs(0x11, ("err",))
    more = np.full(case.S, 140, np.uint32)
    R.drive(case, [more], device=True, monitor=True, sessions=sessions, model=model, init_first=False)
    assert all(np.array_equal(ses.state_words(), b) for ses, b in zip(sessions, before))


def test_the_monitor_after_every_call_equals_fx_kv_execute(gpu):
    case = KS.monitor_case(KS.ABOVE)
    small = KS.monitor_case(64)
    for c in (case, small):
        sessions = None
        model = None
        for i, nexec in enumerate(R.cuts_of_64(c) + [c.nexec]):
            sessions, model = R.drive(c, [nexec], device=True, sessions=sessions, model=model, init_first=(i == 0),
                                      before_launch=poisoner(*FILLS[i % len(FILLS)]))
            mon = sessions[1].monitor(fill=R.FILL, before_launch=poisoner(*FILLS[i % len(FILLS)]))
            whole = fd.run_kv(c.order, nexec, c.key, c.ops, c.S, c.steps, c.keys, c.omax, c.key_mask, fill=R.FILL)
            R.same("the session's monitor", mon, whole, "%s, call %d" % (c.name, i),
                   ("result", "store", "monitor", "mon_off", "err"))
        c.check(mon)


# ------------------------------------------------------------------ contract edges
def both(sessions, case, nexec, **kw):
    host, dev = [ses.advance(case.order, nexec, case.key, case.ops, case.key_mask,
                             before_launch=poisoner(*FILLS[0]), **kw) for ses in sessions]
    R.same("the device", dev, host, "advance")
    return host


def states(sessions):
    return [ses.state_words() for ses in sessions]


def same_states(sessions, before):
    return all(np.array_equal(a, b) for a, b in zip(states(sessions), before))


def unchanged(res, first):
    return all(np.array_equal(np.ravel(getattr(res, f)), np.ravel(getattr(first, f))) for f in ("result", "store", "rank"))


@pytest.mark.parametrize("keys", [5, KS.ABOVE])
def test_calls_that_are_refused_for_a_stream_leave_its_state(gpu, keys):
    """No new rows, a shorter nexec, nexec > steps, then other steps, keys and omax than the session's: err
    alone is written, and the proper call behind them continues the session."""
    case = rand_case(65, keys, 1, 3)
    nexec = R.cut_pairs(case, 4)[1]
    sessions, model = R.drive(case, [nexec], device=True)
    first, before = sessions[0].result(), states(sessions)
    for ses in sessions:
        ses.fill_outputs(0x11, ("err",))
    odd = nexec.copy()
    shrunk, over = np.flatnonzero(nexec > 0)[::3], np.arange(1, case.S, 5)
    odd[shrunk] -= 1
    odd[over] = case.steps + 1
    want = np.zeros(case.S, np.uint32)
    want[shrunk], want[over] = INVALID, OVERFLOW
    res = both(sessions, case, odd)
    assert np.array_equal(res.err, want) and unchanged(res, first) and same_states(sessions, before)
    for change in (dict(steps=case.steps - 1), dict(keys=keys + 1), dict(omax=2)):
        ops = np.concatenate([case.ops, case.ops]) if "omax" in change else case.ops
        res = [ses.advance(case.order, case.nexec, case.key, ops, case.key_mask, **change) for ses in sessions]
        R.same("the device", res[1], res[0], str(change))
        assert np.all(res[0].err == INVALID) and unchanged(res[0], first) and same_states(sessions, before)
    model.call(odd, False)
    R.drive(case, [case.nexec], device=True, monitor=True, sessions=sessions, model=model, init_first=False)


def test_a_state_that_never_saw_init(gpu):
    case = rand_case(65, 5, 1, 4)
    sessions = [K.KvSession(case.S, case.steps, case.keys, case.omax, fill=R.FILL, host=h) for h in (True, False)]
    before = states(sessions)
    res = both(sessions, case, case.nexec, init=False)
    assert np.all(res.err == INVALID) and np.all(res.result == A5) and np.all(res.store == A5) and np.all(res.rank == A5)
    assert same_states(sessions, before)
    mons = [ses.monitor(fill=R.FILL) for ses in sessions]
    R.same("the device's monitor", mons[1], mons[0], "no init", R.MONITOR_FIELDS)
    assert np.all(mons[0].err == INVALID) and np.all(mons[0].mon_off == A5)


def test_init_on_a_used_state_equals_a_fresh_session(gpu):
    used, other = rand_case(65, 5, 1, 5), rand_case(65, 5, 1, 6)
    sessions, _ = R.drive(used, R.cuts_of_64(used)[:2], device=True)
    for ses in sessions:
        ses.fill_outputs(R.FILL)
    fresh, _ = R.drive(other, cuts_63_64_65(other), device=True)
    R.drive(other, cuts_63_64_65(other), device=True, monitor=True, sessions=sessions, model=R.Model(other))
    R.same("the used session", sessions[1].result(), fresh[1].result(), "after FX_FLAG_INIT")
    assert np.array_equal(sessions[1].state_words(), fresh[1].state_words())


# ------------------------------------------------------------------ shapes, fills
@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_block_to_stream_mapping_and_the_tail(gpu, S):
    case = rand_case(S, 65, 1, S)
    R.drive(case, R.cut_pairs(case, 10 + S), device=True, monitor=(S == 130),
            before_launch=poisoner(*FILLS[S % len(FILLS)]))


def test_the_xcd_mapping_of_a_wide_launch(gpu):
    """256 streams and more take the permuted block-to-stream mapping of a padded grid."""
    case = rand_case(300, 5, 1, 300, rows=70)
    R.drive(case, R.cut_pairs(case, 7), device=True, every=False, monitor=True)


@pytest.mark.parametrize("fill", FILLS, ids=str)
def test_every_fill_of_the_register_file(gpu, fill):
    for keys in (65, KS.ABOVE):
        case = rand_case(5, keys, 4, 8)
        R.drive(case, cuts_63_64_65(case), device=True, monitor=True, before_launch=poisoner(*fill))
