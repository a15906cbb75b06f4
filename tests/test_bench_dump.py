"""bench_dump: the arrays `bench.py --dump-outputs` writes (CPU tensors here)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_dump  # noqa: E402
from fantoch_amd import _lib  # noqa: E402


def test_sample_is_fixed_sorted_and_bounded():
    a = bench_dump.sample(1000, bench_dump.SAMPLE_BYTES // 10, 7)
    assert len(a) == 10 and np.all(np.diff(a) > 0) and a.max() < 1000
    assert np.array_equal(a, bench_dump.sample(1000, bench_dump.SAMPLE_BYTES // 10, 7))
    assert np.array_equal(bench_dump.sample(5, 8, 7), np.arange(5))


def test_dump_sim_masks_unwritten_tail_and_keeps_64_bit_counters(tmp_path):
    N, n, cap, R, B = 3, 2, 5, 2, 4
    executed = torch.full((N * n * cap,), -7, dtype=torch.int32)  # -7: never written by a kernel
    el = torch.tensor([[1, 2], [0, 5], [3, 3]], dtype=torch.int32)
    for i in range(N):
        for p in range(n):
            base = (i * n + p) * cap
            executed[base:base + int(el[i, p])] = torch.arange(int(el[i, p]), dtype=torch.int32) + 100 * i + 10 * p
    stats = torch.zeros(N * _lib.FX_SIM_STATS, dtype=torch.int64)
    stats[_lib.FX_SIM_STAT_TRACE] = -0x0123456789abcdef  # a full 64-bit hash
    lat = torch.arange(R * B, dtype=torch.int64).view(R, B)
    bench_dump.dump_sim(torch, str(tmp_path), 1, N, n, cap, executed, el.reshape(-1), lat,
                        torch.ones(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64), stats,
                        torch.zeros(N, dtype=torch.int32))
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["executed_instances"], np.arange(N))
    ex = got["executed"]
    assert ex.shape == (N, n, cap)
    for i in range(N):
        for p in range(n):
            k = int(el[i, p])
            assert np.array_equal(ex[i, p, :k], np.arange(k) + 100 * i + 10 * p) and not ex[i, p, k:].any()
    w = got["stats_words"].astype(np.uint64)
    assert w.shape == (N, 2 * _lib.FX_SIM_STATS)
    t = _lib.FX_SIM_STAT_TRACE
    assert int(w[0, 2 * t]) | (int(w[0, 2 * t + 1]) << 32) == (-0x0123456789abcdef) & (2 ** 64 - 1)
    assert np.array_equal(got["latency_hist"], lat.numpy()) and np.array_equal(got["executed_len"], el.numpy())


def test_dump_executor_reads_the_tiled_planes(tmp_path):
    S, steps = 70, 6  # two tiles, the second ragged; steps no multiple of 4
    pw = _lib.plane_words(S, steps)
    order = torch.full((pw,), -7, dtype=torch.int32)
    release = torch.zeros(pw, dtype=torch.int32)
    nexec = torch.tensor([s % (steps + 1) for s in range(S)], dtype=torch.int32)
    for s in range(S):
        ix = torch.from_numpy(_lib.index(np.arange(steps), s, steps))
        release[ix] = torch.arange(steps, dtype=torch.int32) + 1000 * s
        order[ix[:int(nexec[s])]] = torch.arange(int(nexec[s]), dtype=torch.int32) + 10 * s
    bench_dump.dump_executor(torch, str(tmp_path), 1, S, steps, order, release, nexec,
                             torch.zeros(S, dtype=torch.int32), torch.zeros(4, dtype=torch.int64),
                             torch.zeros(4, dtype=torch.int64))
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert np.array_equal(got["sampled_streams"], np.arange(S))
    assert got["order"].shape == (S, steps) and got["release"].shape == (S, steps)
    for s in range(S):
        k = int(nexec[s])
        assert np.array_equal(got["release"][s], np.arange(steps) + 1000 * s)
        assert np.array_equal(got["order"][s, :k], np.arange(k) + 10 * s) and not got["order"][s, k:].any()
    assert np.array_equal(got["nexec"], nexec.numpy())


def test_plain_and_full_arguments():
    import bench
    import pytest
    plain = bench.parse(["--gpus", "1", "--steps", "2", "--warmup", "0"])
    assert not plain.full and plain.no_cpu_baseline and plain.dump_outputs is None and plain.steps == 2
    full = bench.parse(["--steps", "2", "--warmup", "0", "--full", "--dump-outputs", "d"])
    assert full.full and not full.no_cpu_baseline and full.dump_outputs == "d"
    assert bench.parse(["--full", "--no-cpu-baseline"]).no_cpu_baseline
    assert plain.pmc_key == full.pmc_key  # neither option changes the work of a launch
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--mode", "pred", "--dump-outputs", "d"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)
