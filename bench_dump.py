"""bench.py --dump-outputs DIR: what the timed path computed in its last step,
as DIR/<name>.npy in float64, so that two builds can be compared output for
output (the inputs are seeded: the same arguments give the same batch).

Every array is what a caller of the timed entry point receives.  Integers are
stored exactly: 32-bit words and histogram counts fit a float64, and the
64-bit protocol counters (one is a trace hash) are stored as their two 32-bit
halves.  The large outputs (execution orders) are cut to a fixed sample of
instances / 64-stream tiles, drawn once from a generator seeded with --seed and
stored beside them; positions past an executed length, which the kernels
leave unwritten, are stored as 0.  The whole dump stays under 64 MB.
"""
import os

import numpy as np

LIMIT_BYTES = 64 << 20
SAMPLE_BYTES = 24 << 20  # float64 bytes of one sampled output


def sample(count, row_bytes, seed):
    """Sorted row numbers of a fixed sample of `count` rows of `row_bytes`
    stored bytes each: as many as fit SAMPLE_BYTES (all of them if they do),
    drawn without replacement from a generator seeded with `seed`."""
    k = int(max(1, min(count, SAMPLE_BYTES // max(1, row_bytes))))
    if k >= count:
        return np.arange(count, dtype=np.int64)
    return np.sort(np.random.default_rng(seed).choice(count, k, replace=False)).astype(np.int64)


def write(dirname, arrays):
    """Writes {name: integer or float array} as dirname/<name>.npy in float64."""
    os.makedirs(dirname, exist_ok=True)
    out = {k: np.ascontiguousarray(v).astype(np.float64) for k, v in arrays.items()}
    total = sum(a.nbytes for a in out.values())
    if total > LIMIT_BYTES:
        raise SystemExit("--dump-outputs: %d bytes exceed the %d-byte limit" % (total, LIMIT_BYTES))
    for name, a in out.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    return total


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def dump_sim(torch, dirname, seed, N, n, exec_cap, executed, executed_len, lat_hist, chain, delay, stats, err):
    """fx_sim_run_tiered's outputs of one rank's batch of N instances:
    executed [sample, n, exec_cap] (the sampled instances' per-process
    execution orders, 0 past executed_len) with `executed_instances`, and in
    full executed_len [N, n], the latency / ChainSize / ExecutionDelay
    histograms, stats_words [N, 2 FX_SIM_STATS] (little-endian halves of the
    64-bit counters) and err [N]."""
    pick = sample(N, n * exec_cap * 8, seed)
    idx = torch.from_numpy(pick).to(executed.device)
    el = executed_len.view(N, n)
    live = torch.arange(exec_cap, device=executed.device)[None, None, :] < el[idx][:, :, None]
    ex = torch.where(live, executed.view(N, n, exec_cap)[idx], 0)
    return write(dirname, {
        "executed": _u32(ex),
        "executed_instances": pick,
        "executed_len": _u32(el),
        "latency_hist": lat_hist.cpu().numpy(),
        "chain_size_hist": chain.cpu().numpy(),
        "execution_delay_hist": delay.cpu().numpy(),
        "stats_words": stats.view(N, -1).cpu().numpy().view(np.uint32),
        "err": _u32(err),
    })


def dump_executor(torch, dirname, seed, S, steps, order, release, nexec, err, chain, delay):
    """fx_batch_execute + fx_batch_metrics' outputs of one rank's S streams:
    order / release [sampled streams, steps] (whole 64-stream tiles; order is
    0 past nexec) with `sampled_streams`, and in full nexec [S], err [S] and
    the ChainSize / ExecutionDelay histograms."""
    tiles = (S + 63) // 64
    pick = sample(tiles, 2 * 64 * steps * 8, seed)
    dev = order.device
    streams = (torch.from_numpy(pick).to(dev)[:, None] * 64 + torch.arange(64, device=dev)[None, :]).reshape(-1)
    streams = streams[streams < S]
    step = torch.arange(steps, device=dev)[None, :]
    steps4 = (steps + 3) // 4
    s = streams[:, None]
    pos = ((s >> 6) * steps4 + (step >> 2)) * 256 + ((s & 63) << 2) + (step & 3)  # _lib.index
    live = step < nexec[streams][:, None]
    return write(dirname, {
        "order": _u32(torch.where(live, order[pos], 0)),
        "release": _u32(release[pos]),
        "sampled_streams": streams.cpu().numpy(),
        "nexec": _u32(nexec),
        "err": _u32(err),
        "chain_size_hist": chain.cpu().numpy(),
        "execution_delay_hist": delay.cpu().numpy(),
    })
