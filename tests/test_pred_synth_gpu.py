"""The Caesar commit-stream generator on the device (fx_pred_synth_generate)
against its host twin, byte for byte on poisoned buffers, in both forms of the
kernel; the predecessors executor over the device-generated planes against the
oracle; sessions over them in one and in five pieces; the refusals.  GPU only."""
import ctypes

import numpy as np
import pytest
import torch  # before the library is loaded, as in the benchmarks: one HIP runtime in the process

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import pred as fpred
from fantoch_amd import streams as fs
from oracle import oracle_lib

import pred_synth_shapes as SH

pytestmark = pytest.mark.gpu

POISON = SH.POISON
FORMS = {"library": None, "tile": _lib.FX_PRED_SYNTH_FORM_TILE, "command": _lib.FX_PRED_SYNTH_FORM_COMMAND}
CASES = {name: (kw, with_nd) for name, (kw, _, with_nd) in SH.SHAPES.items()}
CASES["E whole"] = (SH.E_WHOLE, True)
CASES["E part"] = (SH.E_PART, True)
# the jitters of a window above 64 are drawn where they are looked at
CASES["B window 70"] = (dict(SH.SHAPES["B"][0], window=70), True)

_host = {}


def host(name):
    if name not in _host:
        kw, with_nd = CASES[name]
        _host[name] = SH.host_planes(kw, with_nd)
    return _host[name]


def device_buffers(S, steps, dmax):
    bufs = {k: fd.DeviceBuffer(w * 4) for k, w in SH.plane_sizes(S, steps, dmax).items()}
    for b in bufs.values():
        b.fill_bytes(0xA5)
    return bufs


def device_status(lib, kw, bufs, drop=(), form=None):
    p = fpred.pred_synth_params(**kw)
    pl = _lib.PredSynthPlanes(*[None if k in drop else bufs[k].ptr for k in SH.NAMES])
    if form is None:
        st = lib.fx_pred_synth_generate(ctypes.byref(p), ctypes.byref(pl), None)
    else:
        st = lib.fx_pred_synth_generate_form(ctypes.byref(p), ctypes.byref(pl), form, None)
    _lib.check(lib.fx_dev_synchronize(None), "fx_dev_synchronize")
    return st


def downloaded(bufs):
    return {k: b.download(np.uint32, b.nbytes // 4) for k, b in bufs.items()}


def untouched(bufs):
    return all(np.all(a == POISON) for a in downloaded(bufs).values())


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_host_twin(gpu, name, form):
    kw, with_nd = CASES[name]
    S, steps, dmax = fpred.pred_synth_shape(fpred.pred_synth_params(**kw))
    bufs = device_buffers(S, steps, dmax)
    assert device_status(gpu, kw, bufs, () if with_nd else ("ndeps",), FORMS[form]) == _lib.FX_OK
    got, want = downloaded(bufs), host(name)
    for k in SH.NAMES:
        ref = want[k] if want[k] is not None else np.full(got[k].size, POISON, np.uint32)
        diff = np.flatnonzero(got[k] != ref)
        assert diff.size == 0, "%s: %d words differ, the first at %d" % (k, diff.size, diff[0])


def test_equal_stream_slices(gpu):
    whole, part = host("E whole"), host("E part")
    n, steps = SH.E_WHOLE["n"], SH.E_WHOLE["n"] * SH.E_WHOLE["cmds"]
    for s in range(2 * n):
        for k in ("dot", "hdr", "clock_lo", "clock_hi", "ndeps"):
            assert np.array_equal(SH.stream_rows(whole[k], 2 * n + s, steps), SH.stream_rows(part[k], s, steps))


def device_batch(name):
    """Shape `name` generated through pred_synth_device: (host Planes, clock_lo, clock_hi, ndeps)."""
    kw, _ = CASES[name]
    p = fpred.pred_synth_params(**kw)
    S, steps, dmax = fpred.pred_synth_shape(p)
    dev = torch.device("cuda", 0)
    tensors = fpred.pred_synth_device(p, dev, fill=0xA5)
    torch.cuda.synchronize(dev)
    dot, hdr, deps, clo, chi, nd = (t.cpu().numpy().view(np.uint32) for t in tensors)
    want = host(name)
    for got, k in zip((dot, hdr, deps, clo, chi, nd), SH.NAMES):
        assert np.array_equal(got, want[k]), k
    return fs.Planes(S, steps, dmax, kw["n"], dot=dot, hdr=hdr, deps=deps), clo, chi, nd


@pytest.mark.parametrize("name", ["B", "C"])
def test_run_over_device_planes_equals_the_oracle(gpu, name):
    planes, clo, chi, nd = device_batch(name)
    res = fd.run_pred(planes, clo, chi, nd)
    order, release, nexec, err = oracle_lib.pred_batch_execute(planes, clo, chi, threads=2, ndeps=nd)
    assert res.status == _lib.FX_OK
    assert np.array_equal(res.err, err) and np.all(err == 0)
    assert np.array_equal(res.nexec, nexec) and np.all(nexec == planes.steps)
    for s in range(planes.S):
        rows = _lib.index(np.arange(int(nexec[s])), s, planes.steps)
        assert np.array_equal(res.order[rows], order[rows]), "order of stream %d" % s
        rows = _lib.index(np.arange(planes.steps), s, planes.steps)
        assert np.array_equal(res.release[rows], release[rows]), "release of stream %d" % s


def test_sessions_in_one_and_in_five_pieces(gpu):
    planes, clo, chi, nd = device_batch("B")
    tier = _lib.FX_PRED_TIER_LDS
    if gpu.fx_pred_session_bytes(tier, planes.n, planes.dmax, planes.S) == 0:  # FX_ERR_UNSUPPORTED at dmax = 34
        tier = _lib.FX_PRED_TIER_HBM
    results = []
    for pieces in (1, 5):
        ses = fpred.PredSession(planes.S, planes.steps, planes.n, planes.dmax, tier, fill=0xA5)
        for i in range(pieces):
            lens = np.full(planes.S, planes.steps * (i + 1) // pieces, np.uint32)
            res = ses.advance(planes, clo, chi, nd, lens)
        results.append(res)
    one, five = results
    assert np.all(one.err == 0) and np.all(one.nexec == planes.steps)
    for k in fpred.NAMES:
        assert np.array_equal(getattr(one, k), getattr(five, k)), k


@pytest.mark.parametrize("name", sorted(SH.REFUSED))
def test_refused_parameters(gpu, name):
    bufs = device_buffers(64, 64, 4)
    for form in (None, _lib.FX_PRED_SYNTH_FORM_TILE, _lib.FX_PRED_SYNTH_FORM_COMMAND):
        assert device_status(gpu, SH.REFUSED[name], bufs, form=form) == _lib.FX_ERR_INVALID_ARG
    assert untouched(bufs)


def test_refused_planes(gpu):
    for name in ("A", "B"):
        kw, (S, steps, dmax), _ = SH.SHAPES[name]
        bufs = device_buffers(S, steps, dmax)
        for drop in SH.NAMES:
            if drop == "ndeps" and name == "A":
                continue
            assert device_status(gpu, kw, bufs, (drop,)) == _lib.FX_ERR_INVALID_ARG, (name, drop)
        assert device_status(gpu, kw, bufs, form=2) == _lib.FX_ERR_INVALID_ARG
        assert untouched(bufs)
    p = fpred.pred_synth_params(**SH.SHAPES["A"][0])
    assert gpu.fx_pred_synth_generate(ctypes.byref(p), None, None) == _lib.FX_ERR_INVALID_ARG
