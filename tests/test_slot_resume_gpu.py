"""Sessions of the slot executor on the device (fx_slot_advance): in every
test the device equals the host twin byte for byte, and both equal one whole
run over the rows handed over so far (slot_resume.expected_after: slot_ref,
fill included).  Every buffer, the state included, starts as 0xA5 bytes and
the register file is filled with garbage before the launches.  GPU only."""
import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import slot as fslot

import slot_resume as R
import slot_shapes as SS
from test_sim_poison import FILLS, poisoner

pytestmark = pytest.mark.gpu

CASES = SS.all_cases()
IDS = [c.name for c in CASES]
INVALID = _lib.FX_ERR_INVALID_ARG


def pair(case, at_commit=False):
    """The host twin's session and the device's, everything 0xA5."""
    return [fslot.SlotSession(case.S, case.steps, at_commit, fill=SS.FILL, host=h) for h in (True, False)]


def both(sessions, plane, lens, **kw):
    """One call on each side; the results (the host's first), equal in every word."""
    host, dev = [ses.advance(plane, lens, before_launch=poisoner(*FILLS[0]), **kw) for ses in sessions]
    R.same("the device", dev, host, "lengths %s" % (None if lens is None else list(lens[:8])))
    return host, dev


def states(sessions):
    return [ses.state_words() for ses in sessions]


def same_states(sessions, before):
    return all(np.array_equal(a, b) for a, b in zip(states(sessions), before))


@pytest.mark.parametrize("at_commit", [False, True], ids=["", "at commit"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_one_call_equals_the_scan_tier(gpu, i, at_commit):
    case = CASES[i]
    ses = R.drive(case, R.one_call(case), at_commit, device=True, before_launch=poisoner(*FILLS[i % len(FILLS)]))
    scan = fslot.run_slot(case.plane, case.lengths, case.S, case.steps, at_commit, SS.SCAN, fill=SS.FILL)
    R.same("the session", ses[1].result(), scan, case.name)


@pytest.mark.parametrize("cuts", ["64", "pairs 1", "pairs 2"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_cut_streams_after_every_call(gpu, i, cuts):
    """Cuts at the multiples of 64, and per-stream cut pairs: there one call moves different streams by
    different amounts, some by 0."""
    case = CASES[i]
    calls = R.cuts_of_64(case) if cuts == "64" else R.cut_pairs(case, int(cuts[-1]))
    R.drive(case, calls, device=True, before_launch=poisoner(*FILLS[(i + len(cuts)) % len(FILLS)]))


@pytest.mark.parametrize("name", ["flow", "errors", "window edge"])
def test_one_row_per_call(gpu, name):
    """flow: 6 calls; errors: 77; window edge: 130 calls over 4 streams.  In rest(64) and rest(65) slot 64 / 65
    waits from row 0 while the rows behind it execute one per call, each from a saved E that is no multiple
    of 64; the call that brings slot 63 / 64 (rest(65): the cut after row 64) drains two slots.  The reversed
    streams' last row, alone in its call, drains 64 and 65 slots: for 65, two trips of pass B."""
    case = [c for c in CASES if c.name == name][0]
    calls = R.row_per_call(case)
    assert len(calls) == {"flow": 6, "errors": 77, "window edge": 130}[name]
    R.drive(case, calls, device=True, before_launch=poisoner(*FILLS[1]))


def test_a_gap_closer_alone_in_its_call_drains_130_slots(gpu):
    """The reversed stream of 130 slots: 129 rows wait, the last one executes all 130 in three trips of pass B.
    The third stream executes 5 slots first, so its closer drains 125 slots from a saved E of 5 and a saved
    carry of 4: trips that start at no multiple of 64."""
    case = SS.Case("reversed 130", [list(range(130, 0, -1)), [2] + list(range(130, 2, -1)) + [1],
                                    [1, 2, 3, 4, 5] + list(range(130, 6, -1)) + [6]], 130)
    R.drive(case, [R.capped(case, c) for c in (1, 64, 65, 129, 130)], device=True, before_launch=poisoner(*FILLS[2]))
    R.drive(case, R.row_per_call(case)[::3] + [case.lengths], device=True, every=False)


# ------------------------------------------------------------------ hand-written streams, steps 80
# (stream, its lengths in the first, second and third call)
HAND = [
    ([1, 2, 3, 3, 4, 5], (3, 6, 6)),           # the failing row is the first of its call; valid rows behind it
    ([2, 1, 4, 5, 6, 4, 7], (3, 6, 7)),        # the last of its call: a repeat of a slot waiting since call 0
    ([1, 3, 4, 0, 2, 5], (2, 6, 6)),           # a middle row of its call (slot 0 in a later call), valid rows behind
    ([1, 2, 4, 1, 3], (2, 5, 5)),              # a repeat of a slot executed in an earlier call
    ([1, 5, 2, 5, 3], (2, 5, 5)),              # a repeat of a slot waiting since an earlier call
    ([1, 0], (1, 2, 2)),                       # slot 0 alone in a later call
    ([1, 2, 81, 3], (2, 3, 4)),                # a slot above steps: FX_ERR_CAPACITY
    ([2, 81, 2], (1, 3, 3)),                   # ... which comes before the repeat behind it in the same call
    ([80, 1, 2, 3], (1, 2, 4)),                # slot 80 is accepted, and waits
    ([3, 2, 1, 4], (0, 0, 4)),                 # untouched by two calls, then whole
    ([4, 3, 2, 1, 6, 5], (3, 3, 6)),           # closes its gap in the last call
]
FAILING = [0, 1, 2, 3, 4, 5, 6, 7]


def hand_case():
    return SS.Case("hand-written", [st for st, _ in HAND], 80)


def test_hand_written_failures(gpu):
    case = hand_case()
    calls = [np.array([cuts[c] for _, cuts in HAND], np.uint32) for c in range(3)]
    sessions = R.drive(case, calls, device=True, before_launch=poisoner(*FILLS[0]))
    last = sessions[0].result()
    assert [int(x) for x in last.err] == [SS.SLOT] * 6 + [SS.C] * 2 + [0] * 3
    assert [int(x) for x in last.nexec] == [3, 2, 1, 2, 2, 1, 2, 0, 3, 4, 6]
    # the valid rows behind a failing row of the same call keep the fill
    for s, rows in ((0, (3, 4, 5)), (2, (3, 4, 5)), (3, (3, 4)), (6, (2, 3))):
        assert all(int(last.release[_lib.index(a, s, 80)]) == SS.A5 for a in rows)
    assert int(last.release[_lib.index(0, 8, 80)]) == _lib.FX_RELEASE_NONE  # slot 80 waits
    # two more calls with larger lengths for the stopped streams: no word changes; err and nexec are
    # rewritten (they are clobbered first) with the same values
    before = states(sessions)
    for extra in (3, 70):
        lens = calls[2].copy()
        lens[FAILING] += extra
        for ses in sessions:
            ses.fill_outputs(0x11, ("nexec", "err"))
        host, _ = both(sessions, case.plane, lens)
        R.same("the host twin", host, last, "a stopped stream, %d rows more" % extra)
    assert same_states(sessions, before)


# ------------------------------------------------------------------ contract edges
def test_a_call_without_new_rows_rewrites_nexec_and_err(gpu):
    case = SS.window_edge()
    lens = R.capped(case, 70)
    sessions = R.drive(case, [lens], device=True)
    first, before = sessions[0].result(), states(sessions)
    for ses in sessions:
        ses.fill_outputs(0x11, ("nexec", "err"))
    host, _ = both(sessions, case.plane, lens)
    R.same("the host twin", host, first, "len == done")
    assert same_states(sessions, before)


def test_a_shorter_length_is_refused_for_its_stream_and_the_session_continues(gpu):
    case = SS.batch(65)
    lens = R.cut_pairs(case, 4)[1]
    sessions = R.drive(case, [lens], device=True)
    first, before = sessions[0].result(), states(sessions)
    short = lens.copy()
    shrunk = np.flatnonzero(lens > 0)[::2]
    short[shrunk] -= 1
    host, _ = both(sessions, case.plane, short)
    want_err = first.err.copy()
    want_err[shrunk] = INVALID
    assert np.array_equal(host.err, want_err) and np.array_equal(host.nexec, first.nexec)
    assert np.array_equal(host.order, first.order) and np.array_equal(host.release, first.release)
    assert same_states(sessions, before)
    host, _ = both(sessions, case.plane, case.lengths)
    R.same("the host twin", host, R.expected_after(case, case.lengths), "the proper call behind it")


@pytest.mark.parametrize("change", [dict(steps=79), dict(steps=81), dict(execute_at_commit=True)], ids=str)
def test_a_call_that_breaks_the_session_contract(gpu, change):
    """Other steps or the other commit flag: FX_ERR_INVALID_ARG for every stream, the state and every other
    word as they were; the session then goes on."""
    case = SS.errors()
    lens = R.capped(case, 3)
    sessions = R.drive(case, [lens], device=True)
    first, before = sessions[0].result(), states(sessions)
    # the plane of an 80-step batch read with another `steps` is another plane: nothing of it may be read either
    host, _ = both(sessions, case.plane, case.lengths, **change)
    assert np.all(host.err == INVALID) and np.array_equal(host.nexec, first.nexec)
    assert np.array_equal(host.order, first.order) and np.array_equal(host.release, first.release)
    assert same_states(sessions, before)
    host, _ = both(sessions, case.plane, case.lengths)
    R.same("the host twin", host, R.expected_after(case, case.lengths), "the proper call behind it")


@pytest.mark.parametrize("at_commit", [False, True], ids=["", "at commit"])
def test_a_state_that_never_saw_init(gpu, at_commit):
    case = SS.batch(65)
    sessions = pair(case, at_commit)
    before = states(sessions)
    host, _ = both(sessions, case.plane, case.lengths, init=False)
    assert np.all(host.err == INVALID) and np.all(host.nexec == SS.A5)
    assert np.all(host.order == SS.A5) and np.all(host.release == SS.A5)
    assert same_states(sessions, before)


def test_init_on_a_used_state_equals_a_fresh_session(gpu):
    used, other = SS.window_edge(), SS.Case("other", [list(range(130, 0, -1)), [3, 1, 2], [], [2, 2]], 130)
    sessions = R.drive(used, R.cuts_of_64(used)[:2], device=True)
    for ses in sessions:
        ses.fill_outputs(SS.FILL)
    for c in (40, 130):
        lens = R.capped(other, c)
        host, _ = both(sessions, other.plane, lens, init=(c == 40))
        R.same("the host twin", host, R.expected_after(other, lens), "after FX_FLAG_INIT")


# ------------------------------------------------------------------ shapes, modes, fills
@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_block_to_stream_mapping_and_the_tail(gpu, S):
    case = SS.batch(S)
    R.drive(case, R.cut_pairs(case, 10 + S), device=True, before_launch=poisoner(*FILLS[S % len(FILLS)]))


def test_the_xcd_mapping_of_a_wide_launch(gpu):
    """256 streams and more take the permuted block-to-stream mapping of a padded grid."""
    case = SS.flow()
    small = SS.Case("flow 300", case.streams[:300])
    R.drive(small, R.cut_pairs(small, 7), device=True)


@pytest.mark.parametrize("cuts", ["64", "pairs"])
@pytest.mark.parametrize("name", ["errors", "lengths"])
def test_sessions_at_commit(gpu, name, cuts):
    case = [c for c in CASES if c.name == name][0]
    calls = R.cuts_of_64(case) if cuts == "64" else R.cut_pairs(case, 5)
    R.drive(case, calls, at_commit=True, device=True, before_launch=poisoner(*FILLS[1]))


@pytest.mark.parametrize("fill", FILLS, ids=str)
def test_every_fill_of_the_register_file(gpu, fill):
    case = SS.window_edge()
    R.drive(case, R.cut_pairs(case, 6), device=True, before_launch=poisoner(*fill))


# ------------------------------------------------------------------ end to end
def test_generated_streams_in_four_pieces_through_kv_and_pending(gpu):
    """fx_slot_synth_generate -> four fx_slot_advance -> fx_kv_execute, fx_pending_run over the session's
    device-resident order plane: the bytes of the same chain behind fx_slot_run whole."""
    S, steps, window, keys = 65, 200, 100, 16
    plane = fslot.synth_slot(9, S, steps, window, fill=SS.FILL, before_launch=poisoner(*FILLS[0]))
    whole = fslot.run_slot(plane, None, S, steps, fill=SS.FILL, keep_device=True)
    assert np.all(whole.err == 0) and np.all(whole.nexec == steps)
    host_plane = plane.download(np.uint32, whole.plane)
    ses = fslot.SlotSession(S, steps, fill=SS.FILL)
    twin = fslot.SlotSession(S, steps, fill=SS.FILL, host=True)
    lengths = fd.DeviceBuffer(S * 4)
    for piece in range(4):
        lens = np.array([min(steps, 50 * (piece + 1) + s % 7) if piece < 3 else steps for s in range(S)], np.uint32)
        lengths.upload(lens)
        res = ses.advance(plane, lengths, before_launch=poisoner(*FILLS[piece % len(FILLS)]))
        R.same("the device", res, twin.advance(host_plane, lens), "piece %d" % piece)
    R.same("the session", res, whole, "four pieces")
    ops = fd.synth_kv_ops(6, S, steps, read_pct=40, delete_pct=10)
    ones = np.ones(whole.plane, np.uint32)
    got = ses.dev
    for a, b in ((fd.run_kv(got["order"], got["nexec"], plane, ops, S, steps, keys, 1, key_mask=keys - 1, fill=SS.FILL),
                  fd.run_kv(whole.dev["order"], whole.dev["nexec"], plane, ops, S, steps, keys, 1, key_mask=keys - 1,
                            fill=SS.FILL)),
                 (fd.run_pending(got["order"], got["nexec"], plane, ones, S, steps, fill=SS.FILL),
                  fd.run_pending(whole.dev["order"], whole.dev["nexec"], plane, ones, S, steps, fill=SS.FILL))):
        assert np.all(a.err == 0)
        fields = [k for k, v in vars(a).items() if isinstance(v, np.ndarray)]
        assert len(fields) >= 5
        for k in fields:
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
