"""The Caesar commit-stream generator on the host (fx_pred_synth_generate_host)
against pred_synth_ref, the model restated in plain Python, on poisoned
buffers: every plane word, pads included.  Then what the model promises, read
back from the generated planes: every dot once per stream, distinct final
clocks, ascending deps, Caesar's invariant within the horizon, and a complete
run of the oracle's predecessors executor in which every dep with a lower
clock is released no later than its dependent.  The refusals.  No GPU."""
import ctypes

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import pred as fpred
from fantoch_amd import streams as fs
from oracle import oracle_lib

import pred_synth_ref as REF
import pred_synth_shapes as SH

POISON = SH.POISON
ABCD = sorted(SH.SHAPES)

_generated = {}


def generated(name):
    """(keyword arguments, host planes by name, ndeps plane?) of shape `name`, generated once."""
    if name not in _generated:
        kw, _, with_nd = SH.SHAPES[name]
        _generated[name] = (kw, SH.host_planes(kw, with_nd), with_nd)
    return _generated[name]


def batch(name):
    kw, pl, _ = generated(name)
    S, steps, dmax = SH.SHAPES[name][1]
    return fs.Planes(S, steps, dmax, kw["n"], dot=pl["dot"], hdr=pl["hdr"], deps=pl["deps"]), pl


def decoded(name):
    """Per stream: rows of (dot, clock, [deps]) in delivery order."""
    planes, pl = batch(name)
    pw = planes.plane
    out = []
    for s in range(planes.S):
        at = _lib.index(np.arange(planes.steps), s, planes.steps)
        rows = []
        for a in at:
            nd = int(pl["ndeps"][a]) if pl["ndeps"] is not None else (int(pl["hdr"][a]) >> 24) & 31
            rows.append((int(pl["dot"][a]), (int(pl["clock_hi"][a]) << 32) | int(pl["clock_lo"][a]),
                         [int(pl["deps"][k * pw + a]) for k in range(nd)]))
        out.append(rows)
    return out


@pytest.mark.parametrize("name", ABCD)
def test_shape(name):
    kw, want, _ = SH.SHAPES[name]
    assert fpred.pred_synth_shape(fpred.pred_synth_params(**kw)) == want
    assert REF.shape(REF.params(**kw)) == want


@pytest.mark.parametrize("name", ABCD)
def test_host_twin_is_the_restatement(name):
    kw, pl, with_nd = generated(name)
    want = dict(zip(SH.NAMES, REF.generate(REF.params(**kw), ndeps=with_nd)))
    for k in SH.NAMES:
        if want[k] is None:
            assert pl[k] is None
            continue
        assert pl[k].size == want[k].size
        diff = np.flatnonzero(pl[k] != want[k])
        assert diff.size == 0, "%s: %d words differ, the first at %d" % (k, diff.size, diff[0])
    # both left the pads alone and wrote every word in range
    S, steps, _ = SH.SHAPES[name][1]
    at = _lib.index(np.arange(steps)[None, :], np.arange(S)[:, None], steps).reshape(-1)
    pad = np.ones(pl["dot"].size, bool)
    pad[at] = False
    assert pad.any() and np.all(pl["dot"][pad] == POISON) and np.all(pl["clock_hi"][pad] == POISON)


def test_python_entry_points_return_the_same_planes():
    kw, pl, _ = generated("B")
    planes, clo, chi, nd = fpred.pred_synth_host(fpred.pred_synth_params(**kw), fill=0xA5)
    assert (planes.S, planes.steps, planes.dmax, planes.n) == (65, 40, 34, 5)
    for got, k in zip((planes.dot, planes.hdr, planes.deps, clo, chi, nd), SH.NAMES):
        assert np.array_equal(got, pl[k]), k


@pytest.mark.parametrize("name", ABCD)
def test_streams_are_well_formed(name):
    kw = SH.SHAPES[name][0]
    n, cmds = kw["n"], kw["cmds"]
    dots = sorted((s << 24) | j for s in range(1, n + 1) for j in range(1, cmds + 1))
    for rows in decoded(name):
        assert sorted(r[0] for r in rows) == dots
        assert len(set(r[1] for r in rows)) == len(rows)
        for d, clock, deps in rows:
            assert clock & 0xFF == d >> 24
            assert all(a < b for a, b in zip(deps, deps[1:])) and d not in deps


@pytest.mark.parametrize("name", ABCD)
def test_invariant_within_the_horizon(name):
    """Of two commands on one key at most `horizon` rounds apart, the one with
    the lower final clock is in the other's deps."""
    kw = SH.SHAPES[name][0]
    p = REF.params(**kw)
    streams = decoded(name)
    pairs = 0
    for local in range(p.instances):
        inst = REF.Instance(p, local)
        rows = {d: (clock, set(deps)) for d, clock, deps in streams[local * p.n]}
        N = p.n * p.cmds
        for a in range(N):
            for b in range(N):
                ca, cb = rows[inst.dot(a)][0], rows[inst.dot(b)][0]
                if a != b and inst.key[a] == inst.key[b] and ca < cb and inst.round[a] >= inst.round[b] - p.horizon:
                    pairs += 1
                    assert inst.dot(a) in rows[inst.dot(b)][1], (local, a, b)
    assert pairs > 0


def test_the_shapes_hold_what_they_are_for():
    for name in ("B", "C"):
        commit_only, execute_first, later = REF.dep_kinds(REF.params(**SH.SHAPES[name][0]))
        assert commit_only > 0 and execute_first > 0, name
    assert REF.dep_kinds(REF.params(**SH.SHAPES["C"][0]))[2] > 0
    # C: every shared command with a round left is retried
    p = REF.params(**SH.SHAPES["C"][0])
    inst = REF.Instance(p, 1)
    assert all(inst.bump[g] > 0 for g in range(p.n * (p.cmds - 1)) if inst.shared[g])


@pytest.mark.parametrize("name", ABCD)
def test_the_oracle_executes_every_command(name):
    planes, pl = batch(name)
    order, release, nexec, err = oracle_lib.pred_batch_execute(planes, pl["clock_lo"], pl["clock_hi"], threads=2,
                                                               ndeps=pl["ndeps"])
    assert np.all(err == 0) and np.all(nexec == planes.steps)
    for s, rows in enumerate(decoded(name)):
        rel = SH.stream_rows(release, s, planes.steps)
        row_of = {d: i for i, (d, _, _) in enumerate(rows)}
        first = 0
        for i, (d, clock, deps) in enumerate(rows):
            for dep in deps:
                if rows[row_of[dep]][1] < clock:  # an execute-first dep
                    first += 1
                    assert rel[row_of[dep]] <= rel[i], (s, i, dep)
        assert first > 0 or name == "D"


def test_equal_stream_slices():
    """E: instances 2 and 3 of a batch of four are the batch of two at base 2."""
    whole, part = SH.host_planes(SH.E_WHOLE), SH.host_planes(SH.E_PART)
    n, steps = SH.E_WHOLE["n"], SH.E_WHOLE["n"] * SH.E_WHOLE["cmds"]
    _, _, dmax = fpred.pred_synth_shape(fpred.pred_synth_params(**SH.E_WHOLE))
    pw_w, pw_p = _lib.plane_words(4 * n, steps), _lib.plane_words(2 * n, steps)
    for s in range(2 * n):
        for k in ("dot", "hdr", "clock_lo", "clock_hi", "ndeps"):
            assert np.array_equal(SH.stream_rows(whole[k], 2 * n + s, steps), SH.stream_rows(part[k], s, steps)), (k, s)
        for j in range(dmax):
            assert np.array_equal(SH.stream_rows(whole["deps"][j * pw_w:(j + 1) * pw_w], 2 * n + s, steps),
                                  SH.stream_rows(part["deps"][j * pw_p:(j + 1) * pw_p], s, steps)), (j, s)


@pytest.mark.parametrize("name", sorted(SH.REFUSED))
def test_refused_parameters(name):
    kw = SH.REFUSED[name]
    p = fpred.pred_synth_params(**kw)
    S, steps, dmax = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint32(7)
    assert _lib.load().fx_pred_synth_shape(ctypes.byref(p), ctypes.byref(S), ctypes.byref(steps),
                                           ctypes.byref(dmax)) == _lib.FX_ERR_INVALID_ARG
    assert (S.value, steps.value, dmax.value) == (7, 7, 7)
    bufs = SH.host_buffers(64, 64, 4)
    assert SH.host_status(kw, bufs) == _lib.FX_ERR_INVALID_ARG
    assert all(np.all(b == POISON) for b in bufs.values())


@pytest.mark.parametrize("drop", SH.NAMES)
def test_refused_planes(drop):
    """A null plane; ndeps may be NULL when dmax <= 31 (shape A) and not above (shape B)."""
    for name in ("A", "B"):
        kw, (S, steps, dmax), _ = SH.SHAPES[name]
        bufs = SH.host_buffers(S, steps, dmax)
        st = SH.host_status(kw, bufs, (drop,))
        if drop == "ndeps" and name == "A":
            assert st == _lib.FX_OK
            continue
        assert st == _lib.FX_ERR_INVALID_ARG
        assert all(np.all(b == POISON) for b in bufs.values())
    p = fpred.pred_synth_params(**SH.SHAPES["A"][0])
    assert _lib.load().fx_pred_synth_generate_host(ctypes.byref(p), None) == _lib.FX_ERR_INVALID_ARG
    assert _lib.load().fx_pred_synth_generate_host(None, None) == _lib.FX_ERR_INVALID_ARG
