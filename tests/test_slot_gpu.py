"""The slot executor on the device (fx_slot_execute at LANE and at SCAN,
fx_slot_run, fx_slot_synth_generate): every output byte against the host twin
and the restatement of slot.rs (slot_ref), fill included; the KV stage and the
pending stage behind it.  Every buffer, the SCAN tier's state included, starts
as 0xA5 bytes and the register file is filled with garbage before the
launches.  GPU only."""
import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import kv as K
from fantoch_amd import slot as fslot

import kv_ref
import pending_ref
import slot_ref
import slot_shapes as SS
from test_sim_poison import FILLS, poisoner

pytestmark = pytest.mark.gpu

CASES = SS.all_cases()
LADDER = "ladder"  # fx_slot_run with the LANE tier first; None: fx_slot_run as it chooses (SCAN alone)
TIERS = (SS.LANE, SS.SCAN, None, LADDER)
TIER_NAME = {SS.LANE: "lane", SS.SCAN: "scan", None: "run", LADDER: "ladder"}
RUNS = [(i, t, c) for i in range(len(CASES)) for t in TIERS for c in (False, True)]


def run_case(case, tier, at_commit=False, fill=FILLS[0], **kw):
    if tier == LADDER:
        tier, kw = None, dict(kw, lane_first=True)
    return fslot.run_slot(case.plane, case.lengths, case.S, case.steps, at_commit, tier, fill=SS.FILL,
                          before_launch=poisoner(*fill), **kw)


def same_bytes(dev, host):
    for name in fslot.NAMES:
        a, b = getattr(dev, name), getattr(host, name)
        assert np.array_equal(a, b), "%s differs at word %d" % (name, int(np.flatnonzero(a != b)[0]))


@pytest.mark.parametrize("i,tier,at_commit", RUNS, ids=["%s %s%s" % (CASES[i].name, TIER_NAME[t], " at commit" * c)
                                                        for i, t, c in RUNS])
def test_device_equals_host_twin_and_restatement(gpu, i, tier, at_commit):
    case = CASES[i]
    dev = run_case(case, tier, at_commit, FILLS[(i + TIERS.index(tier)) % len(FILLS)])
    case.check(dev, None if tier == LADDER else tier, at_commit)
    if tier is None:
        same_bytes(dev, case.run_host(at_commit))
        assert dev.reruns == 0
    elif tier == LADDER:
        same_bytes(dev, case.run_host(at_commit))
        # the streams that left the lane window (or met a slot above steps), and no others, ran again
        assert dev.reruns == case.reruns(at_commit)
        if not at_commit and case.name in ("lengths", "window edge"):
            assert dev.reruns == sum(case.restated(s, None)["reach"] >= fslot.LANE_WINDOW for s in range(case.S)) > 0
    elif tier == SS.SCAN or case.reruns(at_commit) == 0:  # a tier that stops no stream early leaves the twin's bytes
        same_bytes(dev, case.run_host(at_commit))


def test_stream_map_covers_a_subset(gpu):
    """Lane l of the launch runs stream stream_map[l] (SCAN: on the l-th table); the other streams keep 0xA5."""
    case = SS.batch(130)
    chosen = [129, 3, 64, 0, 77, 63, 5, 128, 65]
    for tier in (SS.LANE, SS.SCAN):
        dev = run_case(case, tier, fill=FILLS[1], stream_map=chosen)
        case.check(dev, tier, only=set(chosen))
    edge = SS.lengths()
    chosen = [s for s in range(edge.S) if s % 6 == 1][::-1]  # the reversed streams, the long ones first
    edge.check(run_case(edge, SS.SCAN, fill=FILLS[2], stream_map=chosen), SS.SCAN, only=set(chosen))


def test_flow_through_the_kv_stage(gpu):
    """slot_executor_flow (slot.rs:132-212): all 720 arrival orders of six slots on one key, Put / Get
    alternating: the Gets return the values of Puts 1, 2, 3, the Puts nothing."""
    flow = SS.flow()
    res = run_case(flow, None, keep_device=True)
    assert np.all(res.err == 0) and np.all(res.nexec == 6)
    ops_of = SS.flow_ops()
    ops, omax = K.pack_kv_ops([[[ops_of[s]] for s in rows] for rows in flow.streams], flow.steps, omax=1)
    kv = fd.run_kv(res.dev["order"], res.dev["nexec"], np.zeros(res.plane, np.uint32), ops, flow.S, flow.steps, 1,
                   omax, fill=SS.FILL)
    assert np.all(kv.err == 0)
    for s, rows in enumerate(flow.streams):
        assert [flow.streams[s][a] for a in res.executed(s)] == [1, 2, 3, 4, 5, 6]
        assert [kv.results(s, rows.index(k))[0] for k in range(1, 7)] == [0, 1, 0, 2, 0, 3]


@pytest.mark.parametrize("window", [8, 100])
def test_generated_streams_never_leave_the_device(gpu, window):
    """fx_slot_synth_generate -> fx_slot_run -> fx_kv_execute -> fx_pending_run over DeviceBuffers only: the
    key of a row is its slot & 15 (the slot plane is the key plane as it is), its op a generated one, its
    rifl its slot, every command one partial."""
    S, steps, keys, base = 130, 150, 16, 9
    lengths = np.array([(11 * s + 1) % (steps + 1) for s in range(S)], np.uint32)
    plane = fslot.synth_slot(4, S, steps, window, lengths, base, fill=SS.FILL, before_launch=poisoner(*FILLS[0]))
    host = fslot.synth_slot_host(4, S, steps, window, lengths, base)
    assert np.array_equal(plane.download(np.uint32, host.size), host)
    res = fslot.run_slot(plane, lengths, S, steps, fill=SS.FILL, before_launch=poisoner(*FILLS[1]), keep_device=True,
                         lane_first=True)
    same_bytes(res, fslot.run_slot_host(host, lengths, S, steps, fill=SS.FILL))
    assert np.all(res.err == 0) and np.array_equal(res.nexec, lengths)
    streams = fslot.unpack_slot_streams(host, lengths, S, steps)
    want_reruns = sum(slot_ref.run(rows, steps, fslot.LANE_WINDOW)["err"] == SS.C for rows in streams)
    assert res.reruns == want_reruns and (want_reruns > 0) == (window > fslot.LANE_WINDOW)
    ops = fd.synth_kv_ops(6, S, steps, read_pct=40, delete_pct=10, lengths=lengths, stream_base=base)
    kv = fd.run_kv(res.dev["order"], res.dev["nexec"], plane, ops, S, steps, keys, 1, key_mask=keys - 1,
                   fill=SS.FILL)
    ones = np.ones(res.plane, np.uint32)
    pend = fd.run_pending(res.dev["order"], res.dev["nexec"], plane, ones, S, steps, fill=SS.FILL)
    assert np.all(kv.err == 0) and np.all(pend.err == 0) and pend.reruns == 0
    hops = ops.download(np.uint32, res.plane)
    for s in (0, 1, 63, 64, 129):
        rows = streams[s]
        order = res.executed(s)
        assert [rows[a] for a in order] == list(range(1, len(rows) + 1))
        op_rows = [[int(x)] for x in hops[_lib.index(np.arange(len(rows)), s, steps)]]
        kv_ref.check_stream(kv, s, order, [k & (keys - 1) for k in rows], op_rows)
        want = pending_ref.run(order, rows, [1] * len(rows), steps)
        assert want["err"] == 0 and pend.ready_heads(s) == want["ready"] == order and int(pend.nopen[s]) == 0


def test_two_arrival_orders_agree_on_every_key(gpu):
    """check_monitors: streams of the same slots in different arrival orders execute the same order per key."""
    L, keys = 120, 8
    streams = [list(range(1, L + 1)), list(range(L, 0, -1))] + [SS.generated(L, w, 21, w) for w in (2, 8, 64, 100)]
    case = SS.Case("orders", streams)
    res = run_case(case, LADDER, keep_device=True)
    assert np.all(res.err == 0) and res.reruns == case.reruns() >= 1
    # a command is named by its slot; slot s writes key s % keys unless s % 3 == 0 (a Get)
    ops, omax = K.pack_kv_ops([[[K.kv_op(K.GET) if s % 3 == 0 else K.kv_op(K.PUT, s)] for s in rows]
                               for rows in streams], case.steps, omax=1)
    kv = fd.run_kv(res.dev["order"], res.dev["nexec"], case.plane, ops, case.S, case.steps, keys, omax,
                   key_mask=keys - 1, fill=SS.FILL, keep_device=True)
    assert np.all(kv.err == 0)
    pairs = [(0, s) for s in range(1, case.S)] + [(3, 5)]
    assert fd.compare_monitors(kv, case.plane, kv, case.plane, pairs) == [(_lib.FX_KV_AGREE, _lib.FX_KV_AGREE)] * len(pairs)
    assert K.monitor_rows(kv, 1, 1) == [L - s for s in range(1, L + 1) if s % keys == 1 and s % 3]


GEN = [(1, 9, 1, False, 0), (65, 44, 8, True, 1000), (2, 257, 64, False, 7), (3, 130, 200, True, 0xFFFFFFF0)]


@pytest.mark.parametrize("S,steps,window,mixed,base", GEN)
def test_generator_equals_host_twin_and_restatement(gpu, S, steps, window, mixed, base):
    lengths = np.array([(5 * s + 1) % (steps + 3) for s in range(S)], np.uint32) if mixed else None
    plane = fslot.synth_slot(3, S, steps, window, lengths, base, fill=SS.FILL, before_launch=poisoner(*FILLS[2]))
    dev = plane.download(np.uint32, _lib.plane_words(S, steps))
    assert np.array_equal(dev, fslot.synth_slot_host(3, S, steps, window, lengths, base, fill=0x3C))
    streams = fslot.synth_slot_streams_c6(3, S, steps, window, lengths, base)
    assert np.array_equal(dev, fslot.pack_slot_streams(streams, steps)[0])  # pad words 0
    for rows in streams:
        assert sorted(rows) == list(range(1, len(rows) + 1))
        assert all(abs(a - (k - 1)) < window for a, k in enumerate(rows))
