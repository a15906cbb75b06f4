"""Sessions of the slot executor on the host (fx_slot_advance_host): for every
partition of a case's streams into calls, every output word after every call
is what one whole run over the rows handed over so far leaves (slot_ref through
slot_shapes, fill included).  The refusals of the entry points.  No GPU."""
import ctypes

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import slot as fslot

import slot_resume as R
import slot_shapes as SS

CASES = SS.all_cases()
IDS = [c.name for c in CASES]
MODES = pytest.mark.parametrize("at_commit", [False, True], ids=["", "at commit"])


@MODES
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_call(case, at_commit):
    R.drive(case, R.one_call(case), at_commit)


@MODES
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_row_per_call(case, at_commit):
    R.drive(case, R.row_per_call(case), at_commit)


@MODES
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cuts_at_multiples_of_64(case, at_commit):
    R.drive(case, R.cuts_of_64(case), at_commit)


@MODES
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cut_pairs_per_stream(case, seed, at_commit):
    calls = R.cut_pairs(case, seed)
    if case.S >= 60:  # the partition has what it is for: empty calls, and streams that move by different amounts
        assert np.any(calls[0] == calls[1]) and np.any(calls[0] == 0) and np.any(calls[1] == case.lengths)
        assert len(set((calls[1] - calls[0]).tolist())) > 2
    R.drive(case, calls, at_commit)


# ------------------------------------------------------------------ the entry points
class Call:
    """One small batch with every pointer valid, for the refusals."""

    def __init__(self):
        self.S, self.steps = 2, 8
        self.plane, self.lengths, _, _ = fslot.pack_slot_streams([[2, 1, 3], [1, 2]], self.steps)
        pw = _lib.plane_words(self.S, self.steps)
        self.out = [np.full(n, SS.A5, np.uint32) for n in (pw, pw, self.S, self.S)]
        self.state = np.full(_lib.load().fx_slot_session_bytes(self.steps, self.S), SS.FILL, np.uint8)
        self.inb = _lib.SlotBatch(self.plane.ctypes.data, self.lengths.ctypes.data, self.S, self.steps)
        self.outb = _lib.OrderBatch(*[a.ctypes.data for a in self.out])

    def host(self, flags=_lib.FX_FLAG_INIT, inb=True, outb=True, state=True):
        return _lib.load().fx_slot_advance_host(ctypes.byref(self.inb) if inb else None,
                                                ctypes.byref(self.outb) if outb else None,
                                                self.state.ctypes.data if state else None, flags)

    def device(self, flags=_lib.FX_FLAG_INIT, inb=True, outb=True, state=True):
        return _lib.load().fx_slot_advance(ctypes.byref(self.inb) if inb else None,
                                           ctypes.byref(self.outb) if outb else None,
                                           self.state.ctypes.data if state else None, flags, None)

    def untouched(self):
        return all(np.all(a == SS.A5) for a in self.out) and bool(np.all(self.state == SS.FILL))


BAD_FLAGS = [_lib.FX_FLAG_SAVE_STATE, 8,_lib.FX_FLAG_INIT | _lib.first_tier_flag(fslot.SCAN), 1 << 31]


@pytest.mark.parametrize("side", ["host", "device"])
def test_refusals_come_before_any_store_or_launch(side):
    """FX_ERR_INVALID_ARG for a null in, out, state or plane pointer, steps >= 2^31 and any flag other than
    INIT and EXECUTE_AT_COMMIT: on the device entry point too, before it looks for a device."""
    c = Call()
    call = getattr(c, side)
    assert call(inb=False) == call(outb=False) == call(state=False) == _lib.FX_ERR_INVALID_ARG
    for flags in BAD_FLAGS:
        assert call(flags=flags) == _lib.FX_ERR_INVALID_ARG
    for field in ("order", "release", "nexec", "err"):
        keep = getattr(c.outb, field)
        setattr(c.outb, field, None)
        assert call() == _lib.FX_ERR_INVALID_ARG
        setattr(c.outb, field, keep)
    c.inb.slot = None
    assert call() == _lib.FX_ERR_INVALID_ARG
    c.inb.slot = c.plane.ctypes.data
    c.inb.steps = 1 << 31
    assert call() == _lib.FX_ERR_INVALID_ARG
    assert c.untouched()


def test_no_device_is_an_error_not_a_fallback(lib):
    """Without a device only: with one this call would launch over host pointers."""
    if lib.fx_device_count() <= 0:
        c = Call()
        assert c.device() == c.device(_lib.FX_FLAG_EXECUTE_AT_COMMIT) == _lib.FX_ERR_NO_DEVICE
        c.inb.num_streams = 0  # the device check comes before the empty batch's FX_OK
        assert c.device() == _lib.FX_ERR_NO_DEVICE
        assert c.untouched()


def test_nothing_to_do_is_ok():
    c = Call()
    c.inb.num_streams = 0
    assert c.host() == _lib.FX_OK
    c.inb.num_streams, c.inb.steps = 2, 0
    assert c.host() == _lib.FX_OK
    assert c.untouched()


def test_lengths_null_means_steps_rows_and_lengths_above_steps_are_capped():
    steps = 5
    plane, _, S, _ = fslot.pack_slot_streams([[3, 2, 1, 5, 4], [1, 2, 3, 4, 5]], steps)
    want = fslot.run_slot_host(plane, None, S, steps, fill=SS.FILL)
    a = fslot.SlotSession(S, steps, fill=SS.FILL, host=True)
    a.launch(plane, np.array([2, 9], np.uint32))
    R.same("a session", a.advance(plane, None), want, "lengths NULL")
    b = fslot.SlotSession(S, steps, fill=SS.FILL, host=True)
    R.same("a session", b.advance(plane, np.array([77, 5], np.uint32)), want, "lengths above steps")


@pytest.mark.parametrize("steps,S", [(1, 1), (64, 3), (65, 2), (1000, 7)])
def test_session_bytes_hold_a_header_and_the_table(steps, S):
    assert _lib.load().fx_slot_session_bytes(steps, S) >= S * (6 + steps) * 4
    assert _lib.load().fx_slot_session_bytes(steps, 0) == 0
