"""GPU graph executor (fantoch_amd/csrc/graph_*.hip behind graph_tiers.hip:
fx_batch_execute, fx_batch_run_tiered) on the edge cases of graph_edges:
every byte of order, release, nexec and err over buffers of 0xA5 bytes.

A stream that fits its tier must equal the C++ oracle in every byte: the
executed rows of order, the release row of each of its Adds (the step, or
FX_RELEASE_NONE for one still pending -- every tier stores that itself), nexec
and err; the rows past its length, the pad rows and pad streams of its tile
and the streams a stream_map leaves out keep 0xA5.  A stream its tier stops
has err == FX_ERR_CAPACITY and what graph_edges.Case.check_stopped defines,
which names per tier what is left open.  fx_batch_run_tiered must leave the
oracle's bytes for every stream, and tier_counts must show that exactly the
streams graph_ref.fits refuses were rerun, and where.  Before every launch
the register file is filled with garbage (test_sim_poison).  GPU only; the
pair conditions and the oracle are in test_graph_edges_ref.py."""
import ctypes

import numpy as np
import pytest

import graph_edges as E
import graph_ref as R
from fantoch_amd import _lib
from fantoch_amd import device as fd
from test_sim_poison import FILLS, poisoner

pytestmark = pytest.mark.gpu

CASES = E.all_cases()
BY = {c.name: c for c in CASES}
FIXED = [(c, t) for c in CASES + E.hbm_cases() for t in c.tiers]
# every case at the tiers above its own too (there all of it fits), the HBM wide tier among them
ABOVE = {E.GROUP: (E.LDS_LARGE, E.WAVE), E.LANE: (E.LDS_LARGE,), E.LANE_REG: (E.GROUP, E.LDS_LARGE),
         E.LDS_LARGE: (E.GLOBAL,), E.WAVE: (E.GLOBAL,), E.GLOBAL: (E.WIDE, E.WIDE_HBM), E.WIDE: (E.WIDE_HBM,),
         E.SPLIT: (E.LDS_LARGE,)}
HIGHER = [(c, t) for c in CASES for t in ABOVE[c.tiers[0]]
          if c.dmax <= R.MAX_DEPS[t] and not (t == E.WIDE_HBM and c.S > 16) and all(c.fits(s, t) for s in range(c.S))]
# the ladder from each of the nine tiers; the batches of more than 16 streams from their own (graph_edges' docstring)
LADDER = [(c, first) for c in CASES for first in (range(_lib.FX_NUM_TIERS) if c.S <= 16 else c.tiers)]


def ident(case, tier):
    return "%s at %s" % (case.name, R.TIER_NAME[tier])


def launch(case, tier, fill=0, **kw):
    return fd.run_batch(case.packed(), tiered=False, tier=tier, metrics=False, order_fill=E.FILL,
                        before_launch=poisoner(*FILLS[fill % len(FILLS)]), **kw)


@pytest.mark.parametrize("case,tier", FIXED, ids=[ident(c, t) for c, t in FIXED])
def test_single_launch_at_the_limits(gpu, case, tier):
    res = launch(case, tier, fill=len(case.name))
    assert res.status == 0
    case.check_launch(res, tier)
    for p in case.pairs:  # err exact per stream: 0 for the fitting half, FX_ERR_CAPACITY for its twin
        assert (res.err[p.fit], res.err[p.exceed]) == (0, _lib.FX_ERR_CAPACITY)


@pytest.mark.parametrize("case,tier", HIGHER, ids=[ident(c, t) for c, t in HIGHER])
def test_single_launch_where_everything_fits(gpu, case, tier):
    assert all(case.fits(s, tier) for s in range(case.S))
    res = launch(case, tier, fill=len(case.name) + 1)
    assert res.status == 0 and not res.err.any()
    case.check_launch(res, tier)


@pytest.mark.parametrize("case,first", LADDER, ids=["%s from %s" % (c.name, R.TIER_NAME[t]) for c, t in LADDER])
def test_ladder_equals_oracle_and_reruns_what_does_not_fit(gpu, case, first):
    res = fd.run_batch(case.packed(), tier=first, metrics=False, order_fill=E.FILL,
                       before_launch=poisoner(*FILLS[first % len(FILLS)]))
    assert res.status == 0
    want = case.expected_ladder()
    for name in E.NAMES:
        a, b = getattr(res, name), want[name]
        assert np.array_equal(a, b), "%s: %s differs at word %d" % (case.name, name, int(np.flatnonzero(a != b)[0]))
    assert res.tier_counts == case.tier_counts(first)


MAPPED = [("placement %s S=130" % R.TIER_NAME[t], t) for t in (E.GROUP, E.LDS_LARGE, E.GLOBAL, E.LANE, E.WAVE,
                                                              E.LANE_REG, E.WIDE)]
MAPPED += [("placement GLOBAL S=65", E.WIDE_HBM)]


@pytest.mark.parametrize("name,tier", MAPPED, ids=["%s at %s" % (n, R.TIER_NAME[t]) for n, t in MAPPED])
def test_stream_map_runs_a_subset_in_any_order(gpu, name, tier):
    """Lane l of the launch runs stream stream_map[l] (the HBM tiers on the l-th block of `state`); the streams
    left out keep 0xA5 in all four outputs."""
    case = BY[name]
    S = case.S
    for chosen in (list(range(S))[::-1], [s for s in range(S) if s % 3 == 1][::-1] + [0], [S - 1], [64, 63, 15, 16]):
        chosen = [s for s in chosen if s < S]
        if tier == E.WIDE_HBM:
            chosen = chosen[:12]
        res = launch(case, tier, stream_map=chosen)
        assert res.status == 0
        case.check_launch(res, tier, streams=chosen)


RESUME = [E.resume_cuts(t) for t in (E.GROUP, E.LDS_LARGE, E.GLOBAL, E.LANE, E.WAVE, E.LANE_REG, E.WIDE_HBM)]


@pytest.mark.parametrize("case,cuts,marks", RESUME, ids=[c.name for c, _, _ in RESUME])
def test_resume_with_full_tables_equals_one_shot(gpu, case, cuts, marks):
    """fx_batch_execute with FX_FLAG_SAVE_STATE over [0, cut), [cut, next) ..: the state saved with every slot
    taken, a window word (and the whole window) full, a vertex with exactly C cached deps and waiters registered
    must carry on to the one-shot result, which is the oracle's.  Every tier at its own sizes (marks: the rows,
    test_graph_edges_ref.py checks what is full there), FX_TIER_WIDE_HBM with 16384 vertices and 32768 bits."""
    tier = case.tiers[0]
    planes = case.packed()
    lib = _lib.load()
    S, steps, pw = planes.S, planes.steps, planes.plane
    dev = [fd.DeviceBuffer(a.nbytes) for a in (planes.dot, planes.hdr, planes.deps, planes.lengths)]
    for b, a in zip(dev, (planes.dot, planes.hdr, planes.deps, planes.lengths)):
        b.upload(a)
    outs = [fd.DeviceBuffer(pw * 4), fd.DeviceBuffer(pw * 4), fd.DeviceBuffer(S * 4), fd.DeviceBuffer(S * 4)]
    state = fd.DeviceBuffer(lib.fx_batch_state_bytes(tier, planes.n, S))
    for b in outs + [state]:
        b.fill_bytes(E.FILL)
    inb = _lib.StreamBatch(dev[0].ptr, dev[1].ptr, dev[2].ptr, dev[3].ptr, S, steps, planes.dmax, planes.n)
    outb = _lib.OrderBatch(*[b.ptr for b in outs])
    rows = [0] + [c for c in cuts if 0 < c < steps] + [steps]
    for a, b in zip(rows[:-1], rows[1:]):
        poisoner(*FILLS[a % len(FILLS)])(None)
        flags = _lib.FX_FLAG_SAVE_STATE | (_lib.FX_FLAG_INIT if a == 0 else 0)
        _lib.check(lib.fx_batch_execute(ctypes.byref(inb), ctypes.byref(outb), tier, None, S, state.ptr, a, b, flags,
                                        None, None))
    _lib.check(lib.fx_dev_synchronize(None), "sync")
    want = case.expected_ladder()
    for name, buf in zip(E.NAMES, outs):
        got = buf.download(np.uint32, pw if name in ("order", "release") else S)
        assert np.array_equal(got, want[name]), "%s: %s differs at word %d" % (
            case.name, name, int(np.flatnonzero(got != want[name])[0]))
