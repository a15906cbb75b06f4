"""Shapes of the Caesar commit-stream generator's tests (test infrastructure):
the parameter sets A to E, the refused ones, and helpers that run a generator
entry point on poisoned buffers of exactly the stated sizes."""
import ctypes

import numpy as np

from fantoch_amd import _lib
from fantoch_amd import pred as fpred

import pred_synth_ref as REF

POISON = REF.POISON

# name -> (keyword arguments of pred_synth_params / pred_synth_ref.params, (S, steps, dmax), ndeps plane?)
SHAPES = {
    # ndeps NULL (dmax <= 31), one conflict rate, no retries
    "A": (dict(seed=11, n=5, instances=3, cmds=3, window=2, horizon=1, max_bump=0, retry_pct=30, conflicts=(100,)),
          (15, 15, 9), False),
    # two stream tiles, ndeps required, three conflict rates
    "B": (dict(seed=12, n=5, instances=13, cmds=8, window=8, horizon=4, max_bump=2, retry_pct=40,
               conflicts=(0, 50, 100)), (65, 40, 34), True),
    # every shared command retried, the whole history in reach, no delivery jitter
    "C": (dict(seed=13, n=3, instances=2, cmds=16, window=0, horizon=15, max_bump=3, retry_pct=100,
               conflicts=(50, 100)), (6, 48, 56), True),
    # the widest row, mostly zero fill
    "D": (dict(seed=14, n=8, instances=1, cmds=2, window=8, horizon=28, max_bump=3, retry_pct=30, conflicts=(50,)),
          (8, 16, 255), True),
}
# E: 4 instances at base 0 against 2 at base 2
E_WHOLE = dict(seed=15, n=5, instances=4, instance_base=0, cmds=6, window=4, horizon=2, max_bump=1, retry_pct=50,
               conflicts=(50, 100))
E_PART = dict(E_WHOLE, instances=2, instance_base=2)

# refused parameter sets: name -> keyword arguments (small planes are handed over: nothing may be stored)
REFUSED = {
    "dmax 263": dict(SHAPES["D"][0], horizon=29),
    "n 0": dict(SHAPES["A"][0], n=0),
    "n 9": dict(SHAPES["A"][0], n=9),
    "cmds 0": dict(SHAPES["A"][0], cmds=0),
    "retry 101": dict(SHAPES["B"][0], retry_pct=101),
    "steps + window 2^24": dict(SHAPES["A"][0], n=5, cmds=3355443, window=1),
    "instance_base + instances 2^32": dict(SHAPES["A"][0], instances=1, instance_base=0xFFFFFFFF),
}
NAMES = ("dot", "hdr", "deps", "clock_lo", "clock_hi", "ndeps")


def plane_sizes(S, steps, dmax):
    pw = _lib.plane_words(S, steps)
    return dict(dot=pw, hdr=pw, deps=max(dmax, 1) * pw, clock_lo=pw, clock_hi=pw, ndeps=pw)


def host_buffers(S, steps, dmax):
    return {k: np.full(w, POISON, np.uint32) for k, w in plane_sizes(S, steps, dmax).items()}


def host_status(kw, bufs, drop=()):
    """fx_pred_synth_generate_host over host buffers, the planes in `drop` handed over as NULL."""
    p = fpred.pred_synth_params(**kw)
    pl = _lib.PredSynthPlanes(*[None if k in drop else bufs[k].ctypes.data for k in NAMES])
    return _lib.load().fx_pred_synth_generate_host(ctypes.byref(p), ctypes.byref(pl))


def host_planes(kw, ndeps=True):
    """The host twin's planes on poisoned buffers, by name (ndeps None without one)."""
    S, steps, dmax = fpred.pred_synth_shape(fpred.pred_synth_params(**kw))
    bufs = host_buffers(S, steps, dmax)
    assert host_status(kw, bufs, () if ndeps else ("ndeps",)) == _lib.FX_OK
    if not ndeps:
        assert np.all(bufs["ndeps"] == POISON)
        bufs["ndeps"] = None
    return bufs


def stream_rows(plane, s, steps):
    """Rows 0 .. steps - 1 of stream s of a plane."""
    return plane[_lib.index(np.arange(steps), s, steps)]
