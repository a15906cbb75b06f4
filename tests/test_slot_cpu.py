"""The slot executor without a GPU: the host twin (fx_slot_execute_host) against
the restatement of slot.rs (slot_ref) on every case, whole planes, fill
included; the argument checks; the generator's host twin against its Python
restatement and against what a generated stream must be."""
import ctypes

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import kv as K
from fantoch_amd import slot as fslot

import kv_ref
import slot_ref
import slot_shapes as SS

CASES = SS.all_cases()


@pytest.mark.parametrize("at_commit", [False, True], ids=["", "at commit"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.name for c in CASES])
def test_host_twin_equals_the_restatement(lib, i, at_commit):
    case = CASES[i]
    res = case.run_host(at_commit)
    assert res.status == 0
    case.check(res, None, at_commit)


def test_the_restatement_on_the_cases_it_is_known_for():
    flow = SS.flow()
    for s in range(flow.S):  # slot.rs:132-212: every permutation executes in slot order
        r = flow.restated(s, None)
        assert [flow.streams[s][a] for a in r["order"]] == [1, 2, 3, 4, 5, 6] and r["err"] == 0
        assert all(r["release"][a] == max(flow.streams[s].index(k) for k in range(1, flow.streams[s][a] + 1))
                   for a in range(6))
    edge = SS.window_edge()
    assert [edge.restated(s, None)["reach"] for s in range(4)] == [63, 64, 63, 64]
    assert [edge.restated(s, SS.LANE)["err"] for s in range(4)] == [0, SS.C, 0, SS.C]
    assert all(edge.restated(s, SS.SCAN)["err"] == 0 and edge.restated(s, SS.SCAN)["nexec"] == len(edge.streams[s])
               for s in range(4))
    holes = SS.holes()
    for s, k in enumerate((1, 20, 40)):
        r = holes.restated(s, None)
        assert r["nexec"] == k - 1 and r["err"] == 0
        assert all((v == slot_ref.NONE) == (holes.streams[s][a] > k) for a, v in r["release"].items())
    err = SS.errors()
    want = [(SS.SLOT, SS.SLOT), (SS.SLOT, SS.SLOT), (SS.SLOT, SS.SLOT), (SS.SLOT, SS.SLOT), (SS.C, SS.SLOT),
            (SS.C, SS.C), (SS.C, SS.C), (SS.SLOT, SS.SLOT), (SS.SLOT, SS.SLOT), (SS.C, SS.C), (SS.SLOT, SS.SLOT)]
    assert [(err.restated(s, SS.LANE)["err"], err.restated(s, SS.SCAN)["err"]) for s in range(err.S)] == want
    assert err.restated(4, SS.SCAN)["nexec"] == 2 and err.restated(10, None)["release"] == \
        {0: slot_ref.NONE, 1: slot_ref.NONE, 2: slot_ref.NONE, 3: 3, 4: 4}
    # at commit only slot 0 fails
    assert [err.restated(s, None, True)["err"] for s in range(err.S)] == \
        [SS.SLOT, SS.SLOT, 0, 0, 0, 0, 0, SS.SLOT, SS.SLOT, SS.SLOT, 0]
    # the lengths case reruns exactly its reversed streams of more than 64 slots
    assert SS.lengths().reruns() == sum(L > 64 for L in SS.LENGTHS)


def test_flow_through_the_kv_stage_on_the_host(lib):
    """slot_executor_flow's results: the Gets return the values of Puts 1, 2, 3, the Puts nothing."""
    flow = SS.flow()
    res = flow.run_host()
    ops_of = SS.flow_ops()
    ops, omax = K.pack_kv_ops([[[ops_of[s]] for s in rows] for rows in flow.streams], flow.steps, omax=1)
    kv = K.run_kv_host(res.order, res.nexec, np.zeros(res.plane, np.uint32), ops, flow.S, flow.steps, 1, omax)
    assert np.all(kv.err == 0)
    for s, rows in enumerate(flow.streams):
        assert [kv.results(s, rows.index(k))[0] for k in range(1, 7)] == [0, 1, 0, 2, 0, 3]
        kv_ref.check_stream(kv, s, res.executed(s), [0] * 6, [[ops_of[k]] for k in rows])
        assert int(kv.store[s, 0]) == 3


def test_argument_checks(lib):
    plane, lengths, S, steps = fslot.pack_slot_streams([[1, 2], [2, 1]])
    out = fslot._filled(S, steps, 0)
    ptrs = [out[n].ctypes.data for n in fslot.NAMES]
    ok_in = _lib.SlotBatch(plane.ctypes.data, lengths.ctypes.data, S, steps)
    ok_out = _lib.OrderBatch(*ptrs)
    bad = _lib.FX_ERR_INVALID_ARG
    assert lib.fx_slot_execute_host(ctypes.byref(ok_in), ctypes.byref(ok_out), 0) == 0
    assert lib.fx_slot_execute_host(None, ctypes.byref(ok_out), 0) == bad
    assert lib.fx_slot_execute_host(ctypes.byref(ok_in), None, 0) == bad
    assert lib.fx_slot_execute_host(ctypes.byref(_lib.SlotBatch(None, None, S, steps)), ctypes.byref(ok_out), 0) == bad
    for i in range(4):
        p = list(ptrs)
        p[i] = None
        assert lib.fx_slot_execute_host(ctypes.byref(ok_in), ctypes.byref(_lib.OrderBatch(*p)), 0) == bad
    assert lib.fx_slot_execute_host(ctypes.byref(ok_in), ctypes.byref(ok_out), _lib.FX_FLAG_INIT) == bad
    big = _lib.SlotBatch(plane.ctypes.data, None, S, 1 << 31)
    assert lib.fx_slot_execute_host(ctypes.byref(big), ctypes.byref(ok_out), 0) == bad
    # the device entry points refuse the same before they look for a device
    assert lib.fx_slot_execute(None, ctypes.byref(ok_out), None, 0, fslot.LANE, None, 0, None) == bad
    assert lib.fx_slot_run(None, ctypes.byref(ok_out), 0, None, None) == bad
    assert lib.fx_slot_run(ctypes.byref(ok_in), ctypes.byref(ok_out), _lib.first_tier_flag(2), None, None) == bad
    assert lib.fx_slot_execute(ctypes.byref(ok_in), ctypes.byref(ok_out), None, 0, 2, None, 0, None) == bad
    assert lib.fx_slot_execute(ctypes.byref(ok_in), ctypes.byref(ok_out), None, 0, fslot.SCAN, None, 0, None) == bad
    assert lib.fx_slot_execute(ctypes.byref(ok_in), ctypes.byref(ok_out), None, 0, fslot.LANE, ptrs[0], 0, None) == bad
    assert lib.fx_slot_execute(ctypes.byref(ok_in), ctypes.byref(ok_out), None, S + 1, fslot.LANE, None, 0,
                               None) == bad
    # the generator
    assert lib.fx_slot_synth_generate_host(1, 0, S, steps, None, 0, plane.ctypes.data) == bad
    assert lib.fx_slot_synth_generate_host(1, 0, S, steps, None, 4, None) == bad
    assert lib.fx_slot_synth_generate_host(1, 0xFFFFFFFF, 2, steps, None, 4, plane.ctypes.data) == bad
    assert lib.fx_slot_synth_generate(1, 0, S, steps, None, 0, plane.ctypes.data, None) == bad
    assert lib.fx_slot_state_bytes(1000, 3) == 3 * 1024 * 4 and lib.fx_slot_state_bytes(0, 3) == 0
    assert lib.fx_status_string(_lib.FX_ERR_SLOT) not in (b"unknown", b"")


GEN = [(1, 9, 1, None, 0), (3, 37, 2, None, 5), (65, 44, 8, "mixed", 1000), (2, 257, 64, None, 7),
       (2, 130, 200, "mixed", 0xFFFFFFF0)]


@pytest.mark.parametrize("S,steps,window,lengths,base", GEN)
def test_generator_host_twin_equals_its_restatement(lib, S, steps, window, lengths, base):
    if lengths is not None:
        lengths = np.array([(5 * s + 1) % (steps + 3) for s in range(S)], np.uint32)  # some beyond steps: capped
    plane = fslot.synth_slot_host(3, S, steps, window, lengths, base, fill=SS.FILL)
    streams = fslot.synth_slot_streams_c6(3, S, steps, window, lengths, base)
    want, want_len, _, _ = fslot.pack_slot_streams(streams, steps)
    assert np.array_equal(plane, want)  # pad words 0 included
    for s, rows in enumerate(streams):
        L = steps if lengths is None else min(int(lengths[s]), steps)
        assert sorted(rows) == list(range(1, L + 1))
        assert all(abs(a - (k - 1)) < window for a, k in enumerate(rows))
        r = slot_ref.run(rows, steps)
        assert r["err"] == 0 and r["nexec"] == L and r["reach"] < window
