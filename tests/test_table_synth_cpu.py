"""The seeded Tempo stream generator on the host (fx_table_synth_shape,
fx_table_synth_lengths_host, fx_table_synth_generate_host) against its
restatement in plain Python (fantoch_amd.table.synth_table_streams_c6), the
argument checks, the struct layouts, and the restatement against the table
executor's restatement (tests/table_ref_mk.py).  No GPU.

cmds * min(kmax, keys) * n below 2^32 is implied by the other limits
(cmds < 2^24, kmax <= 8, n <= 16), so no case can reach that check alone."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import table as ft

import table_ref_mk as RM
import table_synth_shapes as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5A5A5A5


def vote_planes(p, j):
    return p.votes[j * p.plane:(j + 1) * p.plane]


@pytest.mark.parametrize("name", sorted(TS.GEOMS))
def test_host_bytes_match_the_restatement(name):
    """Stream for stream after decoding, on lengths, word for word against
    pack_table_streams on the planes both have, and zero everywhere a stream
    does not reach (rows at or past its length, the pad streams of a tile)."""
    p = TS.params(name)
    ref = TS.restated(name)
    host = ft.synth_table_host(p)
    want = ft.pack_table_streams(ref, p.n, p.keys)
    assert (host.S, host.steps, host.vmax) == (p.streams, want.steps, p.fast_quorum)
    assert host.lengths.tolist() == [len(st) for st in ref]
    for s in range(p.streams):
        assert host.stream(s) == ref[s], "stream %d" % s
    assert (host.nkeys is not None) == (p.kmax > 1)
    for plane in ("hdr", "dot", "clock"):
        assert np.array_equal(getattr(host, plane), getattr(want, plane)), plane
    for j in range(3 * host.vmax):
        w = vote_planes(want, j) if j < 3 * want.vmax else np.zeros(host.plane, np.uint32)
        assert np.array_equal(vote_planes(host, j), w), "votes plane %d" % j
    reached = np.zeros(host.plane, bool)
    for s, st in enumerate(ref):
        reached[_lib.index(np.arange(len(st)), s, host.steps)] = True
    if host.nkeys is not None:
        assert not host.nkeys[~reached].any()
        assert np.array_equal(host.nkeys[reached] != 0, (host.hdr[reached] >> 31) == _lib.FX_TABLE_ATTACHED)


def test_some_stream_length_is_no_multiple_of_four():
    assert any(len(st) % 4 for st in TS.restated("s65_n5_k2"))
    assert any(len(st) % 4 for st in TS.restated("s65_n5_k1_late"))


def test_kmax_one_is_the_single_key_shape():
    for st in TS.restated("s65_n5_k1_late") + TS.restated("s1_n3_keys1"):
        assert all(len(ev) == 5 for ev in st if ev[0] == "A")


def test_conflict_block_splits_the_rates():
    """conflict_block = 32 from stream_base 1000: global streams 1000..1023
    have rate conflicts[(g // 32) % 2] = conflicts[1], 1024..1055 conflicts[0]."""
    kw = dict(TS.GEOMS["s65_n5_k2"], seed=TS.SEED, stream_base=TS.BASE, keys=16, kmax=1)
    kw["conflicts"] = (0, 100)
    p = ft.table_synth_params(**kw)
    for s in (0, 23, 24, 55, 56, 64):
        rate = (0, 100)[((TS.BASE + s) // 32) % 2]
        keys = {ev[1] for ev in ft.synth_table_streams_c6(p, s)}
        assert (keys == {0}) == (rate == 100), s
        assert (0 not in keys) == (rate == 0), s


@pytest.mark.parametrize("name", ["s65_n5_k2", "n16_keys33_k3"])
def test_stream_base(name):
    """Stream s from stream_base b is stream 0 from stream_base b + s (the multi-GPU split)."""
    ref = TS.restated(name)
    for s in (1, len(ref) - 1):
        one = ft.synth_table_host(TS.params(name, streams=1, stream_base=TS.BASE + s))
        assert one.stream(0) == ref[s]
    moved = ft.synth_table_host(TS.params(name, stream_base=TS.BASE + 1))
    assert moved.stream(0) == ref[1] and moved.stream(0) != ref[0]


@pytest.mark.parametrize("name", sorted(TS.GEOMS))
def test_streams_are_well_formed(name):
    p = TS.params(name)
    bound, vmax = ft.table_synth_shape(p)
    assert bound == p.cmds * min(p.kmax, p.keys) * p.n and vmax == p.fast_quorum
    for st in TS.restated(name):
        assert len(st) <= bound
        ranges, seqs, cmds = {}, {}, set()
        for ev in st:
            votes = ev[4] if ev[0] == "A" else ev[2]
            assert len(votes) == (p.fast_quorum if ev[0] == "A" else 1)
            for voter, start, end in votes:
                ranges.setdefault((ev[1], voter), []).append((start, end))
            if ev[0] == "A":
                cmds.add(ev[2])
                assert 1 <= (ev[5] if len(ev) > 5 else 1) <= min(p.kmax, p.keys)
        for rs in ranges.values():  # per (key, voter): no gap and no overlap, from clock 1 on
            at = 0
            for start, end in sorted(rs):
                assert start == at + 1 and end >= start
                at = end
        assert len(cmds) == p.cmds
        for src, seq in cmds:
            seqs.setdefault(src, []).append(seq)
        for got in seqs.values():  # dots per coordinator count 1, 2, ...
            assert sorted(got) == list(range(1, len(got) + 1))


def sentinel_planes(S, steps, vmax):
    p = ft.TablePlanes(S, steps, 5, 16, vmax)
    arrays = [np.full(p.plane, SENTINEL, np.uint32) for _ in range(4)] + \
        [np.full(3 * vmax * p.plane, SENTINEL, np.uint32), np.full(S, SENTINEL, np.uint32)]
    hdr, dot, clock, nkeys, votes, lengths = arrays
    c = _lib.TableSynthPlanes(hdr.ctypes.data, dot.ctypes.data, clock.ctypes.data, votes.ctypes.data,
                              nkeys.ctypes.data, lengths.ctypes.data)
    return c, arrays


BAD = {
    "n_0": dict(n=0, fast_quorum=0), "n_17": dict(n=17), "fq_0": dict(fast_quorum=0), "fq_above_n": dict(fast_quorum=6),
    "kmax_0": dict(kmax=0), "kmax_9": dict(kmax=_lib.FX_TABLE_MAX_CMD_KEYS + 1), "cmds": dict(cmds=_lib.FX_SEQ_MASK + 1),
    "conflict_101": dict(conflicts=(2, 101)), "keys_0": dict(keys=0), "keys": dict(keys=_lib.FX_TABLE_SYNTH_MAX_KEYS + 1),
    "window": dict(window=_lib.FX_SEQ_MASK + 1), "lag": dict(lag=_lib.FX_SEQ_MASK + 1),
    "stream_base": dict(stream_base=(1 << 32) - 1, streams=2),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_write_nothing(lib, case):
    kw = dict(seed=1, streams=2, n=5, fast_quorum=3, keys=16, cmds=10, kmax=2)
    kw.update(BAD[case])
    p = ft.table_synth_params(**kw)
    steps, vmax = ctypes.c_uint32(77), ctypes.c_uint32(77)
    assert lib.fx_table_synth_shape(ctypes.byref(p), ctypes.byref(steps), ctypes.byref(vmax)) == _lib.FX_ERR_INVALID_ARG
    assert (steps.value, vmax.value) == (77, 77)
    assert lib.fx_table_synth_scratch_bytes(ctypes.byref(p)) == 0
    c, arrays = sentinel_planes(2, 200, 5)
    assert lib.fx_table_synth_generate_host(ctypes.byref(p), ctypes.byref(c), 200) == _lib.FX_ERR_INVALID_ARG
    assert lib.fx_table_synth_lengths_host(ctypes.byref(p), arrays[-1].ctypes.data_as(_lib.u32p), None) == \
        _lib.FX_ERR_INVALID_ARG
    # the device entry points check the arguments before they look for a device
    assert lib.fx_table_synth_generate(ctypes.byref(p), ctypes.byref(c), 200, arrays[0].ctypes.data, None) == \
        _lib.FX_ERR_INVALID_ARG
    assert lib.fx_table_synth_lengths(ctypes.byref(p), arrays[-1].ctypes.data, arrays[0].ctypes.data, None, None) == \
        _lib.FX_ERR_INVALID_ARG
    assert all(np.all(a == SENTINEL) for a in arrays)


def test_missing_planes_are_refused(lib):
    p = ft.table_synth_params(streams=2, cmds=10, kmax=2)
    c, arrays = sentinel_planes(2, 200, 3)
    assert lib.fx_table_synth_generate_host(ctypes.byref(p), None, 200) == _lib.FX_ERR_INVALID_ARG
    for field in ("hdr", "dot", "clock", "votes", "nkeys", "lengths"):
        keep = getattr(c, field)
        setattr(c, field, None)
        assert lib.fx_table_synth_generate_host(ctypes.byref(p), ctypes.byref(c), 200) == _lib.FX_ERR_INVALID_ARG, field
        setattr(c, field, keep)
    assert all(np.all(a == SENTINEL) for a in arrays)
    # nkeys may be missing with single-key commands only
    p1 = ft.table_synth_params(streams=2, cmds=10, kmax=1)
    c.nkeys = None
    assert lib.fx_table_synth_generate_host(ctypes.byref(p1), ctypes.byref(c), 200) == _lib.FX_OK
    assert np.all(arrays[3] == SENTINEL) and not np.any(arrays[0] == SENTINEL)


def test_steps_one_short_is_refused_untouched(lib):
    p = TS.params("s65_n5_k2")
    longest = max(len(st) for st in TS.restated("s65_n5_k2"))
    c, arrays = sentinel_planes(65, longest - 1, 3)
    assert lib.fx_table_synth_generate_host(ctypes.byref(p), ctypes.byref(c), longest - 1) == _lib.FX_ERR_CAPACITY
    assert all(np.all(a == SENTINEL) for a in arrays)
    c, arrays = sentinel_planes(65, longest, 3)
    assert lib.fx_table_synth_generate_host(ctypes.byref(p), ctypes.byref(c), longest) == _lib.FX_OK
    assert not any(np.any(a == SENTINEL) for a in arrays)


def test_shape_and_device_entry_points_without_a_device(lib):
    p = TS.params("s65_n5_k2")
    assert ft.table_synth_shape(p) == (40 * 2 * 5, 3)
    nbytes = lib.fx_table_synth_scratch_bytes(ctypes.byref(p))
    assert nbytes >= 128 * (40 + 6 + 1) * 4  # a counter per slot and stream of the two tiles
    off = TS.params("keys64_n5")
    assert lib.fx_table_synth_scratch_bytes(ctypes.byref(off)) >= 128 * (25 + 6 + 1 + 65 * 5) * 4
    if lib.fx_device_count() <= 0:
        c, arrays = sentinel_planes(65, 400, 3)
        assert lib.fx_table_synth_generate(ctypes.byref(p), ctypes.byref(c), 400, arrays[0].ctypes.data, None) == \
            _lib.FX_ERR_NO_DEVICE
        assert lib.fx_table_synth_lengths(ctypes.byref(p), arrays[-1].ctypes.data, arrays[0].ctypes.data, None,
                                          None) == _lib.FX_ERR_NO_DEVICE
        assert all(np.all(a == SENTINEL) for a in arrays)


PAIRS = {"TableSynthParams": "fx_table_synth_params", "TableSynthPlanes": "fx_table_synth_planes"}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ctypes_mirrors_match_the_header():
    """As tests/test_abi_layout.py, for the structs of the generator."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "fantoch_amd.h"', "int main(void) {"]
    for py, c in PAIRS.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (py, c))
        for name, _ in getattr(_lib, py)._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (py, name, c, name))
    lines += ["  return 0;", "}"]
    d = tempfile.mkdtemp()
    try:
        src, exe = os.path.join(d, "abi.c"), os.path.join(d, "abi")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True,
                       capture_output=True, text=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    finally:
        shutil.rmtree(d, ignore_errors=True)
    layout = {(a, b): int(v) for a, b, v in (ln.split() for ln in out.split("\n") if ln)}
    for py in PAIRS:
        cls = getattr(_lib, py)
        assert ctypes.sizeof(cls) == layout[(py, "size")], py
        for name, _ in cls._fields_:
            assert getattr(cls, name).offset == layout[(py, name)], (py, name)


# (n, keys, kmax, cmds, conflict, lag, window), every one with lag >= window
EXECUTING = [(3, 2, 2, 40, 100, 6, 4), (5, 16, 2, 40, 50, 80, 50), (5, 3, 3, 60, 10, 6, 4), (7, 4, 2, 40, 2, 6, 4),
             (5, 2, 2, 40, 50, 0, 0), (16, 8, 2, 30, 20, 6, 4)]


@pytest.mark.parametrize("n,keys,kmax,cmds,conflict,lag,window", EXECUTING)
def test_restated_streams_execute_in_full(n, keys, kmax, cmds, conflict, lag, window):
    """With lag >= window the executor's restatement executes every attached
    event of 30 streams (the seeds of the existing generator's measurement
    become 30 global streams of one seed)."""
    fq = thr = n // 2 + 1
    p = ft.table_synth_params(seed=3, streams=30, n=n, fast_quorum=fq, keys=keys, cmds=cmds, kmax=kmax,
                              conflicts=(conflict,), lag=lag, window=window)
    for s in range(30):
        st = ft.synth_table_streams_c6(p, s)
        res = RM.run_stream(st, n, thr, keys)
        assert res["err"] == 0, "stream %d" % s
        assert res["nexec"] == sum(ev[0] == "A" for ev in st), "stream %d" % s
