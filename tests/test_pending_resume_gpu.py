"""Sessions of the pending stage on the device (fx_pending_advance): in every
test two sessions, the device's and the host twin's, fed the same calls and
compared byte for byte after every call; the twin against one whole run at
the HBM tier over the same nexec (pending_resume.Model).  Every buffer, the
state included, starts as 0xA5 bytes and the register file is filled with
garbage before the launches.  GPU only."""
import random

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import pending as P

import pending_resume as R
import pending_shapes as PS
from pending_shapes import rifl, singles, stream
from test_sim_poison import FILLS, poisoner

pytestmark = pytest.mark.gpu

INVALID, OVERFLOW = _lib.FX_ERR_INVALID_ARG, _lib.FX_ERR_ORDER_OVERFLOW
A5 = R.A5
MAXP = _lib.FX_PENDING_MAX_PARTS


def rand_case(S, seed, rows=131):
    rng = random.Random(seed)
    return PS.Case("random S%d" % S, [PS.rand_stream(rng, rows, min(rows, rng.choice([0, 1, 63, 64, 65, 129, rows])) if s % 3
                                                     else rows) for s in range(S)], flag_every=3)


def calls_of(cuts):
    return [np.array([c[i] for c in cuts], np.uint32) for i in range(len(cuts[0]))]


@pytest.mark.parametrize("cuts", ["64", "pairs 1", "pairs 2"])
@pytest.mark.parametrize("name", ["pairs and wide", "rifl reuse", "capacity", "hbm buckets", "errors", "process 2"])
def test_cut_streams_after_every_call(gpu, name, cuts):
    case = [c for c in PS.all_cases() if c.name == name][0]
    calls = R.cuts_of_64(case) if cuts == "64" else R.cut_pairs(case, int(cuts[-1]))
    R.drive(case, calls, device=True, before_launch=poisoner(*FILLS[len(cuts) % len(FILLS)]))


def test_commands_that_straddle_calls(gpu):
    X, Y = rifl(7), rifl(8)
    sts = [
        # a command of 2 parts split across a cut
        (stream(singles(9, 100) + [(X, 2)] + singles(30, 200) + [(X, 2)] + singles(5, 300)), (10, 40, 46)),
        # a rifl reused after its command completed in an earlier call
        (stream([(X, 2), (X, 2)] + singles(20, 100) + [(X, 2), (X, 2), (X, 3)] + singles(10, 200) + [(X, 3), (X, 3)]),
         (2, 24, 35)),
        # a count that differs from a builder created in an earlier call: the stream stops at that row
        (stream([(X, 3), (Y, 2)] + singles(20, 100) + [(Y, 2), (X, 2), (X, 3)] + singles(5, 200), err=INVALID),
         (5, 30, 30)),
        # the same with valid rows of the call in front of it and behind it
        (stream([(X, 3)] + singles(70, 100) + [(Y, 2), (X, 2), (Y, 2)], err=INVALID), (1, 66, 74)),
        # a chunk of a call that starts at row 3: builders created at rows 3 .. 66, completed in the next call
        (stream(singles(3, 100) + PS.live(64)), (3, 67, 131)),
    ]
    case = PS.Case("straddling", [st for st, _ in sts], steps=140)
    sessions, model = R.drive(case, calls_of([c for _, c in sts]), device=True, before_launch=poisoner(*FILLS[0]))
    res = sessions[1].result()
    assert [int(x) for x in res.err] == [0, 0, INVALID, INVALID, 0]
    assert [int(x) for x in res.nopen] == [0, 1, 1, 2, 0]
    # the stopped streams stay stopped
    before = [int(x) for x in res.nready]
    R.drive(case, [np.array([46, 37, 30, 74, 131], np.uint32)], device=True, sessions=sessions, model=model,
            init_first=False)
    res = sessions[1].result()
    assert [int(x) for x in res.nready] == before[:1] + [before[1] + 1] + before[2:]
    case.check(res, P.HBM)


def test_a_command_of_max_parts_with_one_part_per_call(gpu):
    X = rifl(7)
    sts = [stream([(X, MAXP)] * MAXP), stream([(X, MAXP)] * (MAXP - 1) + singles(1, 50)),
           stream([(X, MAXP), (rifl(9), 2)] * MAXP)]
    case = PS.Case("max parts", sts)
    sessions, _ = R.drive(case, R.row_per_call(case), device=True, before_launch=poisoner(*FILLS[1]))
    res = sessions[1].result()
    assert [int(x) for x in res.nready] == [1, 1, 1 + MAXP // 2] and [int(x) for x in res.nopen] == [0, 1, 0]
    assert res.parts(0, 0, MAXP) == list(range(MAXP))
    case.check(res, P.HBM)


def test_process_masking_with_a_cut_between_the_rows(gpu):
    for case in PS.masked():
        sessions, _ = R.drive(case, [R.capped(case, c) for c in (1, 2, 3, 30, 31)] + [case.nexec], device=True,
                              before_launch=poisoner(*FILLS[2]))
        case.check(sessions[1].result(), P.HBM)


def test_128_rifls_that_never_complete_take_every_entry(gpu):
    """steps = 128, two buckets, one row per call: every row creates a builder that is live at the end of its
    call, so every call takes an entry and the last one takes the table's last."""
    case = PS.Case("128 live", [stream([(rifl(1 + i), 2) for i in range(128)]),
                                stream([(r, 2) for r in PS.colliding(128, 2)])], steps=128)
    sessions, _ = R.drive(case, R.row_per_call(case), device=True, every=False)
    res = sessions[1].result()
    assert [int(x) for x in res.nopen] == [128, 128] and np.all(res.err == 0) and np.all(res.nready == 0)
    tab = sessions[1].state_words().reshape(case.S, -1)[:, 64:].reshape(case.S, 128, 4)
    for s, st in enumerate(case.streams):
        assert sorted(int(x) for x in tab[s, :, 0]) == sorted(st["rifl_of"])
        assert sorted(int(x) for x in tab[s, :, 1]) == list(range(128))
        assert np.all(tab[s, :, 2] == (0x80000000 | 1 << 8 | 2))  # live, got 1 of 2
    case.check(res, P.HBM)


def test_colliding_rifls_inserted_across_calls(gpu):
    """The probe walks buckets that earlier calls filled, and wraps round."""
    steps = 192
    same, last = PS.colliding(70, 3), PS.colliding(70, 3, 2)
    sts = [stream([(r, 2) for r in same] + singles(50, 100) + [(r, 2) for r in reversed(same)]),
           stream([(r, 2) for r in last] + singles(2, 100) + [(r, 2) for r in last[3:]])]
    case = PS.Case("colliding", sts, steps=steps)
    for calls in ([R.capped(case, c) for c in range(10, steps, 10)] + [case.nexec], R.cut_pairs(case, 2)):
        sessions, _ = R.drive(case, calls, device=True, before_launch=poisoner(*FILLS[0]))
        case.check(sessions[1].result(), P.HBM)


@pytest.mark.parametrize("steps", [63, 65])
def test_one_bucket_and_two(gpu, steps):
    rng = random.Random(steps)
    case = PS.Case("steps %d" % steps, [PS.rand_stream(rng, steps, steps) for _ in range(3)] +
                   [stream(PS.live(steps // 2))], steps=steps)
    assert _lib.pending_buckets(steps) == {63: 1, 65: 2}[steps]
    for calls in (R.cut_pairs(case, steps), [R.capped(case, c) for c in range(7, steps, 7)] + [case.nexec]):
        sessions, _ = R.drive(case, calls, device=True, before_launch=poisoner(*FILLS[1]))
        case.check(sessions[1].result(), P.HBM)


def test_new_ready_on_the_device(gpu):
    case = rand_case(5, 11)
    ses = P.PendingSession(case.S, case.steps, case.count_mask, case.process, fill=R.FILL)
    seen = [[] for _ in range(case.S)]
    for nexec in R.cut_pairs(case, 3):
        res = ses.advance(case.order, nexec, case.rifl, case.count)
        for s in range(case.S):
            seen[s] += ses.new_ready(s)
            assert seen[s] == res.ready_heads(s)


# ------------------------------------------------------------------ contract edges
def both(sessions, case, nexec, **kw):
    host, dev = [ses.advance(case.order, nexec, case.rifl, case.count, before_launch=poisoner(*FILLS[0]), **kw)
                 for ses in sessions]
    R.same("the device", dev, host, "advance")
    return host


def unchanged(res, first):
    return all(np.array_equal(getattr(res, f), getattr(first, f)) for f in P.NAMES if f != "err")


def test_calls_that_are_refused_for_a_stream_leave_its_state(gpu):
    """No new rows, a shorter nexec, nexec > steps, then other steps, count_mask and process than the
    session's: err alone is written, and the proper call behind them continues the session."""
    case = rand_case(65, 3)
    nexec = R.cut_pairs(case, 4)[1]
    sessions, model = R.drive(case, [nexec], device=True)
    first, before = sessions[0].result(), sessions[1].state_words()
    for ses in sessions:
        ses.fill_outputs(0x11, ("err",))
    odd = nexec.copy()
    shrunk, over = np.flatnonzero(nexec > 0)[::3], np.arange(1, case.S, 5)
    odd[shrunk] -= 1
    odd[over] = case.steps + 1
    want = np.zeros(case.S, np.uint32)
    want[shrunk], want[over] = INVALID, OVERFLOW
    res = both(sessions, case, odd)
    assert np.array_equal(res.err, want) and unchanged(res, first)
    assert np.array_equal(sessions[1].state_words(), before)
    for change in (dict(steps=case.steps - 1), dict(count_mask=0xFF), dict(process=1)):
        res = both(sessions, case, case.nexec, **change)
        assert np.all(res.err == INVALID) and unchanged(res, first)
        assert np.array_equal(sessions[1].state_words(), before)
    model.call(odd, False)
    R.drive(case, [case.nexec], device=True, sessions=sessions, model=model, init_first=False)


def test_a_state_that_never_saw_init(gpu):
    case = rand_case(65, 4)
    sessions = [P.PendingSession(case.S, case.steps, fill=R.FILL, host=h) for h in (True, False)]
    before = sessions[1].state_words()
    res = both(sessions, case, case.nexec, init=False)
    assert np.all(res.err == INVALID) and all(np.all(getattr(res, f) == A5) for f in P.NAMES if f != "err")
    assert np.array_equal(sessions[1].state_words(), before)


def test_init_on_a_used_state_equals_a_fresh_session(gpu):
    used, other = rand_case(65, 5), rand_case(65, 6)
    sessions, _ = R.drive(used, R.cuts_of_64(used)[:2], device=True)
    for ses in sessions:
        ses.fill_outputs(R.FILL)
    fresh, _ = R.drive(other, R.cut_pairs(other, 1), device=True)
    R.drive(other, R.cut_pairs(other, 1), device=True, sessions=sessions, model=R.Model(other))
    R.same("the used session", sessions[1].result(), fresh[1].result(), "after FX_FLAG_INIT")


def test_nexec_above_steps_in_the_first_call_is_the_whole_stages_refusal(gpu):
    case = PS.errors()
    sessions, model = R.drive(case, R.one_call(case), device=True)
    whole = fd.run_pending(case.order, case.nexec, case.rifl, case.count, case.S, case.steps, case.count_mask,
                           case.process, fill=R.FILL, tier=P.HBM)
    R.same("the session", sessions[1].result(), whole, case.name)
    ok = case.nexec.copy()
    ok[8] = 100  # a proper call behind the refusal starts at row 0
    R.drive(case, [ok], device=True, sessions=sessions, model=model, init_first=False)
    assert int(sessions[1].result().err[8]) == 0 and int(sessions[1].result().nready[8]) > 0


def test_a_table_entry_that_no_session_wrote_is_no_builder(gpu):
    """A valid header over a table entry whose head row or count is out of range: the look-up passes it by, so no
    index comes from memory unchecked, and the row that would have completed its command creates a builder.  The
    expectations are literal (the kernel's, run on the commit before the look-up was shared with k_pending): the
    host twin drops such an entry when it loads its state and would report nopen = 1."""
    S, steps, X = 4, 64, rifl(7)
    case = PS.Case("bad entries", [stream([(X, 2), (X, 2)]) for _ in range(S)], steps=steps)
    ses = P.PendingSession(S, steps, case.count_mask, case.process, fill=R.FILL)
    res = ses.advance(case.order, np.full(S, 1, np.uint32), case.rifl, case.count)
    assert np.all(res.err == 0) and np.all(res.nopen == 1) and np.all(res.nready == 0)
    state = ses.state_words().reshape(S, -1)
    assert state.shape[1] == 64 + 64 * 4 and np.all(state[:, 6] == 1)  # one bucket; the header's live
    live = 0x80000000 | 1 << 8  # PENDING_LIVE, got 1
    entry = []                  # per stream the first word of the entry {rifl, head row, state word, 0}
    for s in range(S):
        hits = [e for e in range(64, 64 + 64 * 4, 4) if state[s, e + 2] & 0x80000000 and state[s, e] == X]
        assert len(hits) == 1 and [int(w) for w in state[s, hits[0]:hits[0] + 4]] == [X, 0, live | 2, 0]
        entry.append(hits[0])
    state[0, entry[0] + 1] = steps             # head row = steps
    state[1, entry[1] + 2] = live | 1          # count 1
    state[2, entry[2] + 2] = live | (MAXP + 1)  # count FX_PENDING_MAX_PARTS + 1
    ses.state.upload(state)
    res = ses.advance(case.order, np.full(S, 2, np.uint32), case.rifl, case.count, before_launch=poisoner(*FILLS[0]))
    want = {name: np.full(len(getattr(res, name)), A5, np.uint32) for name in P.NAMES}

    def at_row(row, s):
        return int(_lib.index(row, s, steps))

    want["err"][:] = 0
    for s in range(S):
        want["head"][at_row(0, s)] = 0          # call 1: row 0 creates the builder with head row 0
        want["part"][at_row(0, s)] = 0
    for s in range(3):                          # the entry is no builder: row 1 creates one
        want["head"][at_row(1, s)] = 1
        want["part"][at_row(1, s)] = 1          # slot 0 of head row 1
        want["nready"][s], want["nopen"][s] = 0, 2  # the header's live of 1, plus one creator
    want["head"][at_row(1, 3)] = 0              # the entry as call 1 left it: row 1 completes its command
    want["part"][case.plane + at_row(0, 3)] = 1  # slot 1 of head row 0
    want["index"][at_row(0, 3)] = 0
    want["ready"][at_row(0, 3)] = 0
    want["nready"][3], want["nopen"][3] = 1, 0
    R.same("the device", res, want, "bad entries")


# ------------------------------------------------------------------ shapes, fills
@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_block_to_stream_mapping_and_the_tail(gpu, S):
    case = rand_case(S, S)
    R.drive(case, R.cut_pairs(case, 10 + S), device=True, before_launch=poisoner(*FILLS[S % len(FILLS)]))


def test_the_xcd_mapping_of_a_wide_launch(gpu):
    """256 streams and more take the permuted block-to-stream mapping of a padded grid."""
    case = rand_case(300, 300, rows=70)
    R.drive(case, R.cut_pairs(case, 7), device=True, every=False)


@pytest.mark.parametrize("fill", FILLS, ids=str)
def test_every_fill_of_the_register_file(gpu, fill):
    case = PS.reuse()
    R.drive(case, R.cut_pairs(case, 6), device=True, before_launch=poisoner(*fill))
    R.drive(case, R.row_per_call(case)[::5] + [case.nexec], device=True, before_launch=poisoner(*fill))
