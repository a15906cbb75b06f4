"""Sessions of the predecessors executor on the device (fx_pred_advance): in
every test the device equals the host twin byte for byte, and both equal
pred_ref over the rows handed over so far at the tier's limits
(pred_resume.Expect, fill included).  Every buffer, the state included, starts
as 0xA5 bytes and the register file is filled with garbage before the
launches.  The list is test_pred_resume_cpu's, with the device beside the
twin, and the device-only shapes and the end-to-end chain.  GPU only."""
import ctypes
import types

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import pred as fpred
from fantoch_amd import streams as fs

import pred_edges as E
import pred_ref as PRF
import pred_resume as R
import test_pred_resume_cpu as C
from test_sim_poison import FILLS, poisoner

pytestmark = pytest.mark.gpu

SMALL, LDS, HBM = R.SMALL, R.LDS, R.HBM
MODES = C.MODES


def poison(i=0):
    return poisoner(*FILLS[i % len(FILLS)])


def states(sessions):
    return [ses.state_words() for ses in sessions]


def same_states(sessions, before):
    return all(np.array_equal(a, b) for a, b in zip(states(sessions), before))


def both(sessions, case, lens, **kw):
    """One call on each side; the host's result, which the device equals in every word."""
    host, dev = [ses.advance(*R.batch(case), lens, before_launch=poison(), **kw) for ses in sessions]
    R.same("the device", dev, host, "lengths %s" % (None if lens is None else list(lens[:8])))
    return host


# ------------------------------------------------------------------ whole runs and cuts
@MODES
@pytest.mark.parametrize("i", range(len(C.RUNS)), ids=C.RUN_IDS)
def test_one_call_equals_the_whole_run(gpu, i, at_commit):
    case, tier = C.RUNS[i]
    ses = R.drive(case, R.one_call(case), tier, at_commit, device=True, before_launch=poison(i))
    planes, clo, chi, nd = R.batch(case)
    whole = fd.run_pred(planes, clo, chi, nd, execute_at_commit=at_commit, tier=tier, fill=R.FILL)
    R.same("the session", ses[1].result(), whole, case.name)


@pytest.mark.parametrize("i", range(len(C.ON_CHIP)), ids=C.ON_CHIP_IDS)
def test_cut_after_every_4_rows(gpu, i):
    case, tier = C.ON_CHIP[i]
    R.drive(case, R.cuts_of(case, 4), tier, device=True, before_launch=poison(i))


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("i", range(len(C.ON_CHIP)), ids=C.ON_CHIP_IDS)
def test_cut_pairs_per_stream(gpu, i, seed):
    """One call moves different streams by different amounts, some by 0."""
    case, tier = C.ON_CHIP[i]
    R.drive(case, R.cut_pairs(case, seed), tier, device=True, before_launch=poison(i + seed))


@pytest.mark.parametrize("i", range(len(C.HBM_ONLY)), ids=[c.name for c in C.HBM_ONLY])
def test_hbm_only_cases_cut_at_three_places(gpu, i):
    case = C.HBM_ONLY[i]
    R.drive(case, R.three_cuts(case, HBM), HBM, device=True, before_launch=poison(i))


@pytest.mark.parametrize("i", range(len(C.PAIRS)), ids=C.PAIR_IDS)
def test_reachable_limits_one_row_before_the_stop(gpu, i):
    """As on the host: the exceeding stream stops in the later call; two further calls with larger lengths
    rewrite nexec and err (clobbered first) and change nothing else, the state included."""
    case, pair = C.PAIRS[i]
    tier = pair.tier
    calls = R.cut_before_stop(case, pair, tier)
    sessions = R.drive(case, calls, tier, device=True, before_launch=poison(i))
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


@pytest.mark.parametrize("i", range(len(C.ONE_ROW)), ids=C.ONE_ROW_IDS)
def test_one_row_per_call_and_committed_and_executed(gpu, i):
    case, tier = C.ONE_ROW[i]
    R.drive(case, R.row_per_call(case), tier, device=True, before_launch=poison(i), executed=True)


@pytest.mark.parametrize("name,tier", [("deps count", SMALL), ("deps count", LDS), ("deps count", HBM),
                                       ("deps header", SMALL), ("deps header", LDS)])
def test_deps_beyond_the_tile_row_cut_after_every_row(gpu, name, tier):
    case = C.named(name)
    R.drive(case, R.row_per_call(case), tier, device=True, before_launch=poison(tier))


@pytest.mark.parametrize("compiled,tier", [(False, SMALL), (False, LDS), (False, HBM), (True, SMALL)],
                         ids=["SMALL", "LDS", "HBM", "compiled"])
def test_hand_built_streams_across_a_cut(gpu, compiled, tier):
    R.check_hand_streams_hold_registrations()
    case = R.hand_case(compiled)
    sessions = R.drive(case, R.hand_calls(), tier, device=True, before_launch=poison(tier))
    last = sessions[1].result()
    assert [int(x) for x in last.err] == R.HAND_ERR
    assert [int(x) for x in last.nexec] == R.HAND_NEXEC


# ------------------------------------------------------------------ contract edges
def started(case, tier, lens, at_commit=False):
    sessions = R.drive(case, [lens], tier, at_commit, device=True, before_launch=poison())
    return sessions, sessions[0].result(), states(sessions)


def continues(sessions, case, tier, at_commit=False):
    lens = R.lengths_of(case)
    R.same("the host twin", both(sessions, case, lens), R.expected_after(case, lens, tier, at_commit),
           "the proper call behind it")


def test_a_call_without_new_rows_rewrites_nexec_and_err(gpu):
    case, tier = C.named("lengths"), SMALL
    lens = R.capped(case, 5)
    sessions, first, before = started(case, tier, lens)
    for ses in sessions:
        ses.fill_outputs(0x11, ("nexec", "err"))
    R.same("the host twin", both(sessions, case, lens), first, "len == done")
    assert same_states(sessions, before)
    continues(sessions, case, tier)


def test_a_shorter_length_is_refused_for_its_stream_and_the_session_continues(gpu):
    case, tier = C.named("lengths compiled"), SMALL
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


@pytest.mark.parametrize("which", range(6), ids=["steps - 1", "steps + 1", "commit flag", "tier", "dmax + 1", "no ndeps"])
@pytest.mark.parametrize("name,tier", [("lengths", SMALL), ("lengths compiled", SMALL), ("errors", LDS)])
def test_a_call_that_breaks_the_session_contract(gpu, name, tier, which):
    """FX_ERR_INVALID_ARG for every stream, the state and every other word as they were; the session goes on."""
    case = C.named(name)
    change = C.contract_changes(case, tier)[which]
    sessions, first, before = started(case, tier, R.capped(case, 3))
    host = both(sessions, case, R.lengths_of(case), **change)
    assert np.all(host.err == R.INVALID) and np.array_equal(host.nexec, first.nexec)
    assert np.array_equal(host.order, first.order) and np.array_equal(host.release, first.release)
    assert same_states(sessions, before)
    continues(sessions, case, tier)


@MODES
@pytest.mark.parametrize("tier", [SMALL, LDS, HBM], ids=["SMALL", "LDS", "HBM"])
def test_a_state_that_never_saw_init(gpu, tier, at_commit):
    """0xA5 everywhere: nothing is written but err, and no garbage count indexes anything."""
    case = C.named("lengths")
    sessions = R.sessions_of(case, tier, at_commit, device=True)
    before = states(sessions)
    assert all(np.all(w == R.A5) for w in before)
    host = both(sessions, case, R.lengths_of(case), init=False)
    assert np.all(host.err == R.INVALID) and np.all(host.nexec == R.A5)
    assert np.all(host.order == R.A5) and np.all(host.release == R.A5)
    assert same_states(sessions, before)


@pytest.mark.parametrize("word,value", [(6, 1 << 20), (8, 1000), (9, 65)], ids=["done > steps", "nexec > done", "nfree > P"])
def test_a_header_with_a_count_out_of_range_is_refused(gpu, word, value):
    case, tier = C.named("lengths"), SMALL
    sessions, first, _ = started(case, tier, R.capped(case, 3))
    for ses in sessions:
        C.corrupt(ses, word, value)
    before = states(sessions)
    host = both(sessions, case, R.lengths_of(case))
    assert np.all(host.err == R.INVALID) and np.array_equal(host.nexec, first.nexec)
    assert np.array_equal(host.order, first.order) and np.array_equal(host.release, first.release)
    assert same_states(sessions, before)


def test_init_on_a_used_state_equals_a_fresh_session(gpu):
    used = C.named("lengths")
    other = E.Case("other", used.n, used.streams[::-1], used.tiers)
    sessions = R.drive(used, R.cuts_of(used, 4)[:2], SMALL, device=True, before_launch=poison())
    for ses in sessions:
        ses.fill_outputs(R.FILL)
    for c in (4, 9):
        lens = R.capped(other, c)
        R.same("the host twin", both(sessions, other, lens, init=(c == 4)), R.expected_after(other, lens, SMALL),
               "after FX_FLAG_INIT")


# ------------------------------------------------------------------ shapes and fills, device only
@pytest.mark.parametrize("S", [1, 3, 4, 5, 63, 64, 65, 130])
def test_four_streams_per_workgroup_and_the_tail(gpu, S):
    case = E.lanes5(S)
    R.drive(case, R.cut_pairs(case, 10 + S), SMALL, device=True, before_launch=poison(S))


@pytest.mark.parametrize("compiled", [False, True], ids=["generic", "compiled"])
def test_the_xcd_mapping_of_a_wide_launch(gpu, compiled):
    """300 streams: 256 and more take the permuted block-to-stream mapping of a padded grid (compiled: 75
    workgroups of four, the identity mapping, beside it)."""
    if compiled:
        case = E.Case("lanes compiled 300", 5, [E.mixed(7 * s, (5 * s + 2) % 14, 5, 5) for s in range(300)], [SMALL], 5)
    else:
        case = E.Case("many 300", 3, [E.mixed(300 + s, (3 * s + 1) % 11, 3, 3) for s in range(300)], [SMALL, LDS])
    R.drive(case, R.cut_pairs(case, 7), SMALL, device=True, before_launch=poison(1))


def test_1200_streams_of_the_compiled_layout_take_the_permuted_mapping(gpu):
    """Four streams per workgroup: 1,200 streams are 300 workgroups, a padded and permuted grid."""
    case = E.Case("lanes compiled 1200", 5, [E.mixed(3 * s, (5 * s + 2) % 9, 5, 5) for s in range(1200)], [SMALL], 5)
    R.drive(case, R.cut_pairs(case, 3), SMALL, device=True, every=False, before_launch=poison(2))


@pytest.mark.parametrize("fill", FILLS, ids=str)
def test_every_fill_of_the_register_file(gpu, fill):
    for case in (C.named("lengths compiled"), C.named("lengths")):
        R.drive(case, R.cut_pairs(case, 6), SMALL, device=True, before_launch=poisoner(*fill))


# ------------------------------------------------------------------ end to end
def test_generated_streams_in_four_pieces_through_kv(gpu):
    """fx_synth_generate (n = 5, 65 streams, 40 commands per process, the Caesar clocks of bench_pred.py) -> four
    fx_pred_advance at SMALL -> fx_kv_execute over the session's device-resident order plane: the bytes of the
    same chain behind one fx_pred_execute at the same tier."""
    lib = _lib.load()
    p = fs.synth_params(seed=2, instances=13, n=5, cmds=40, conflicts=(2, 50))
    S, steps, dmax = fs.synth_shape(p)
    assert (S, steps, dmax) == (65, 200, 5)
    pw, keys = _lib.plane_words(S, steps), 16
    dot, hdr, deps = fd.DeviceBuffer(pw * 4), fd.DeviceBuffer(pw * 4), fd.DeviceBuffer(pw * dmax * 4)
    poison()(None)
    _lib.check(lib.fx_synth_generate(ctypes.byref(p), dot.ptr, hdr.ptr, deps.ptr, None), "fx_synth_generate")
    _lib.check(lib.fx_dev_synchronize(None), "sync")
    host = fs.Planes(S, steps, dmax, 5, dot.download(np.uint32, pw), hdr.download(np.uint32, pw),
                     deps.download(np.uint32, pw * dmax))
    clo_h = ((host.dot & np.uint32(0xFFFFFF)) << np.uint32(8)) | ((host.dot >> np.uint32(24)) & np.uint32(0xFF))
    chi_h = np.zeros_like(clo_h)
    keep = []
    clo, chi = fd._dev(clo_h, keep), fd._dev(chi_h, keep)
    # whole, device-resident
    whole = {name: fd.DeviceBuffer(k * 4) for name, k in zip(R.NAMES, (pw, pw, S, S))}
    for b in whole.values():
        b.fill_bytes(R.FILL)
    base = _lib.StreamBatch(dot.ptr, hdr.ptr, deps.ptr, None, S, steps, dmax, 5)
    inb = _lib.PredBatch(base, clo.ptr, chi.ptr, None)
    outb = _lib.OrderBatch(*[whole[name].ptr for name in R.NAMES])
    _lib.check(lib.fx_pred_execute(ctypes.byref(inb), ctypes.byref(outb), None, S, SMALL, None, 0, None),
               "fx_pred_execute")
    _lib.check(lib.fx_dev_synchronize(None), "sync")
    whole_h = types.SimpleNamespace(**{name: whole[name].download(np.uint32, whole[name].nbytes // 4)
                                       for name in R.NAMES})
    assert np.all(whole_h.err == 0) and np.all(whole_h.nexec == steps)  # no stream stops at SMALL
    ses = fpred.PredSession(S, steps, 5, dmax, SMALL, fill=R.FILL)
    twin = fpred.PredSession(S, steps, 5, dmax, SMALL, fill=R.FILL, host=True)
    dev_planes = types.SimpleNamespace(dot=dot, hdr=hdr, deps=deps)
    lengths = fd.DeviceBuffer(S * 4)
    for piece in range(4):
        lens = np.array([min(steps, 50 * (piece + 1) + s % 7) if piece < 3 else steps for s in range(S)], np.uint32)
        lengths.upload(lens)
        res = ses.advance(dev_planes, clo, chi, None, lengths, before_launch=poison(piece))
        R.same("the device", res, twin.advance(host, clo_h, chi_h, None, lens), "piece %d" % piece)
    R.same("the session", res, whole_h, "four pieces")
    ops = fd.synth_kv_ops(6, S, steps, read_pct=40, delete_pct=10)
    got = ses.dev
    a = fd.run_kv(got["order"], got["nexec"], dot, ops, S, steps, keys, 1, key_mask=keys - 1, fill=R.FILL)
    b = fd.run_kv(whole["order"], whole["nexec"], dot, ops, S, steps, keys, 1, key_mask=keys - 1, fill=R.FILL)
    assert np.all(a.err == 0)
    fields = [k for k, v in vars(a).items() if isinstance(v, np.ndarray)]
    assert len(fields) >= 3
    for k in fields:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
