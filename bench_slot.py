"""FPaxos's SlotExecutor on the GPU over batched streams (fx_slot_run).

Workload: `--streams` streams of `--slots` slots each, generated on the device
(fx_slot_synth_generate: a leader that commits in slot order, MChosen reordered
by less than `--window` positions), every stream distinct, nothing uploaded.

One step = fx_slot_run over every stream (`--tier run`: as it chooses, the SCAN
tier alone; `--tier ladder`: the LANE tier, then the streams that leave its
64-slot window again on the SCAN tier), or with `--tier lane|scan` one
fx_slot_execute at that tier; wall clock around the call and a synchronise.  A
sample of streams is downloaded, compared with the Python restatement of the
generator (fantoch_amd.slot.synth_slot_streams_c6) and checked bit for bit
against the restatement of slot.rs (tests/slot_ref.py).  Prints one JSON line
and appends it to profiles/slot_bench.json with `--record`.

`--kv [--read-pct P] [--delete-pct D]` adds the KV stage: after each step one
fx_kv_execute over the step's own order plane, the slot plane as the key plane
(key = slot & (keys - 1)) and one generated op per row; `--pending` adds
fx_pending_run with the slot plane as the rifl plane and a count plane of ones.
Both are timed beside the step (kv_ms, pending_ms), not in it, and the sampled
streams are checked against tests/kv_ref.py and tests/pending_ref.py.

`--chunks N` times a session instead (fx_slot_advance): the same streams fed in
N equal pieces, N calls and one synchronise per step, the first piece of every
step with FX_FLAG_INIT; beside it, step by step in turn, one fx_slot_execute at
the SCAN tier over the whole streams, for the ratio.  The line goes to
profiles/slot_resume_bench.json with `--record`.

`--host` also times fx_slot_execute_host over the same streams on `--threads`
threads (whole plane tiles per thread), for information."""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBPS = 8000.0


def measured_copy_gbps(nbytes=1 << 30, reps=10):
    """Achievable HBM bandwidth in this session: a device-to-device copy of nbytes, read + written bytes per second."""
    import torch
    dev = torch.device("cuda", 0)
    a = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize(dev)
    return 2.0 * nbytes * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9


def chunks_bench(args, plane, gen_ms, copy):
    """--chunks N: one step = N fx_slot_advance calls over one session, piece i
    bringing every stream to ceil(slots * (i + 1) / N) rows, the first with
    FX_FLAG_INIT, then one synchronise; wall clock around all of it.  Beside it,
    alternating step by step in the same process, one fx_slot_execute at the
    SCAN tier over the whole streams, for the ratio.  The sampled streams'
    outputs after the last piece are checked against tests/slot_ref.py."""
    from fantoch_amd import _lib
    from fantoch_amd import device as fd
    from fantoch_amd import slot as fslot
    import slot_ref
    lib = _lib.load()
    S, steps, N = args.streams, args.slots, args.chunks
    pw = _lib.plane_words(S, steps)
    ses = fslot.SlotSession(S, steps)
    ses.out["order"].zero()
    ses.out["release"].fill_bytes(0xFF)
    cuts = [(steps * (i + 1) + N - 1) // N for i in range(N)]
    lengths = []
    for c in cuts:
        lengths.append(fd.DeviceBuffer(S * 4))
        lengths[-1].upload(np.full(S, c, np.uint32))
    outb = _lib.OrderBatch(*(ses.out[name].ptr for name in fslot.NAMES))
    batches = [_lib.SlotBatch(plane.ptr, l.ptr, S, steps) for l in lengths]

    def step():
        t1 = time.time()
        for i, b in enumerate(batches):
            _lib.check(lib.fx_slot_advance(ctypes.byref(b), ctypes.byref(outb), ses.state.ptr,
                                           _lib.FX_FLAG_INIT if i == 0 else 0, None), "fx_slot_advance")
        _lib.check(lib.fx_dev_synchronize(None), "sync")
        return 1e3 * (time.time() - t1)

    whole = {name: fd.DeviceBuffer(n * 4) for name, n in zip(fslot.NAMES, (pw, pw, S, S))}
    whole["order"].zero()
    whole["release"].fill_bytes(0xFF)
    whole_in = _lib.SlotBatch(plane.ptr, None, S, steps)
    whole_out = _lib.OrderBatch(*(whole[name].ptr for name in fslot.NAMES))
    scan_state = fd.DeviceBuffer(lib.fx_slot_state_bytes(steps, S))

    def scan_step():
        t1 = time.time()
        _lib.check(lib.fx_slot_execute(ctypes.byref(whole_in), ctypes.byref(whole_out), None, S, fslot.SCAN,
                                       scan_state.ptr, 0, None), "fx_slot_execute")
        _lib.check(lib.fx_dev_synchronize(None), "sync")
        return 1e3 * (time.time() - t1)

    for _ in range(max(args.warmup, 1)):
        step()
        scan_step()
    ms, scan_ms = [], []
    for _ in range(args.steps):
        ms.append(step())
        scan_ms.append(scan_step())

    res = {name: ses.out[name].download(np.uint32, ses.out[name].nbytes // 4) for name in fslot.NAMES}
    ref_out = {name: whole[name].download(np.uint32, whole[name].nbytes // 4) for name in fslot.NAMES}
    equal_scan = all(np.array_equal(res[name], ref_out[name]) for name in fslot.NAMES)
    host_plane = plane.download(np.uint32, pw)
    parity, checked = True, 0
    for j in range(args.sample):
        s = (j * 977 + 13) % S
        at = _lib.index(np.arange(steps), s, steps)
        slots = [int(x) for x in host_plane[at]]
        parity = parity and slots == fslot.synth_slot_streams_c6(args.seed, 1, steps, args.window, stream_base=s)[0]
        ref = slot_ref.run(slots, steps, None)
        want_r = np.full(steps, _lib.FX_RELEASE_NONE, np.uint32)
        for a, v in ref["release"].items():
            want_r[a] = v
        ok = (int(res["err"][s]) == ref["err"] and int(res["nexec"][s]) == ref["nexec"]
              and [int(x) & 0x7FFFFFFF for x in res["order"][at][:ref["nexec"]]] == ref["order"]
              and np.array_equal(res["release"][at], want_r))
        parity, checked = parity and ok, checked + 1

    rows = S * steps
    step_ms, scan_step_ms = sum(ms) / len(ms), sum(scan_ms) / len(scan_ms)
    alg_bytes = 12.0 * rows
    achieved = alg_bytes / (step_ms * 1e-3) / 1e9
    line = {
        "metric": "rows/sec, FPaxos SlotExecutor session (fx_slot_advance, %d pieces per step)" % N,
        "value": round(rows / (step_ms * 1e-3), 1), "unit": "rows/s", "higher_is_better": True,
        "ms_per_step": round(step_ms, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
        "includes": "%d fx_slot_advance calls (the first with FX_FLAG_INIT) and one synchronise (wall clock)" % N,
        "chunks": N, "rows_per_piece": cuts[0], "steps": args.steps, "warmup": args.warmup, "n_gpus": 1, "dtype": "u32",
        "window": args.window,
        "scan_whole_ms_per_step": round(scan_step_ms, 3),
        "scan_whole_ms_min_max": [round(min(scan_ms), 3), round(max(scan_ms), 3)],
        "ratio_to_scan_whole": round(step_ms / scan_step_ms, 3),
        "errors": int(np.count_nonzero(res["err"])), "rows_per_step": rows,
        "executed_per_step": int(res["nexec"].astype(np.uint64).sum()),
        "config": {"streams": S, "slots_per_stream": steps, "seed": args.seed,
                   "parallelism": "a wavefront per stream and call"},
        "roofline": {"bound": "hbm", "alg_bytes_per_step": int(alg_bytes),
                     "alg_bytes_definition": "12 B per row: one slot word read, one order word and one release word "
                                             "written",
                     "achieved_gbps": round(achieved, 3), "copy_gbps_same_session": round(copy, 1) if copy else None,
                     "frac_of_copy": round(achieved / copy, 5) if copy else None,
                     "peak": HBM_PEAK_GBPS, "frac_of_peak": round(achieved / HBM_PEAK_GBPS, 6)},
        "generation_ms": round(min(gen_ms[1:]), 3),
        "equals_scan_whole": bool(equal_scan), "sample_parity": bool(parity), "sample_streams": checked,
    }
    print(json.dumps(line), flush=True)
    if args.record:
        path = os.path.join(ROOT, "profiles", "slot_resume_bench.json")
        lines = json.load(open(path))["lines"] if os.path.exists(path) else []
        lines.append({"args": " ".join(sys.argv[1:]), "line": line})
        with open(path, "w") as f:
            json.dump({"what": "bench_slot.py --chunks lines, one per invocation (--record); ms_per_step is wall time "
                               "around the N fx_slot_advance calls of a step and one synchronise, "
                               "scan_whole_ms_per_step the same around one fx_slot_execute at SCAN, step by step "
                               "in turn in the same process", "lines": lines}, f, indent=1)
            f.write("\n")
    return 0 if parity and equal_scan else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=20480)
    ap.add_argument("--slots", type=int, default=1000)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--tier", choices=("run", "ladder", "lane", "scan"), default="run")
    ap.add_argument("--kv", action="store_true")
    ap.add_argument("--keys", type=int, default=16, help="--kv: a power of two")
    ap.add_argument("--read-pct", type=int, default=50)
    ap.add_argument("--delete-pct", type=int, default=10)
    ap.add_argument("--pending", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sample", type=int, default=8)
    ap.add_argument("--no-copy", action="store_true", help="skip the copy-bandwidth measurement")
    ap.add_argument("--record", action="store_true",
                    help="append the line to profiles/slot_bench.json (--chunks: profiles/slot_resume_bench.json)")
    ap.add_argument("--chunks", type=int, default=0,
                    help="N > 0: the streams fed in N equal pieces through one session (fx_slot_advance)")
    args = ap.parse_args()
    if args.chunks < 0 or args.chunks > max(args.slots, 1):
        raise SystemExit("--chunks must lie in 0 .. --slots")
    if args.chunks and (args.tier != "run" or args.kv or args.pending or args.host):
        raise SystemExit("--chunks times the session alone (and the SCAN tier whole beside it): no --tier, --kv, "
                         "--pending, --host")

    # (torch initialises the device before the library is loaded, as in bench.py)
    copy = None if args.no_copy else measured_copy_gbps()
    from fantoch_amd import _lib
    from fantoch_amd import device as fd
    from fantoch_amd import slot as fslot
    import slot_ref
    lib = _lib.load()
    if lib.fx_device_count() <= 0:
        raise SystemExit("no GPU visible to libfantoch_amd")
    if args.keys & (args.keys - 1):
        raise SystemExit("--keys must be a power of two")
    S, steps = args.streams, args.slots
    pw = _lib.plane_words(S, steps)

    gen_ms = []
    plane = fd.DeviceBuffer(pw * 4)
    for _ in range(3):  # (the first is a warm-up)
        t1 = time.time()
        _lib.check(lib.fx_slot_synth_generate(args.seed, 0, S, steps, None, args.window, plane.ptr, None), "generate")
        _lib.check(lib.fx_dev_synchronize(None), "sync")
        gen_ms.append(1e3 * (time.time() - t1))

    if args.chunks:
        return chunks_bench(args, plane, gen_ms, copy)

    out = {name: fd.DeviceBuffer(n * 4) for name, n in zip(fslot.NAMES, (pw, pw, S, S))}
    out["order"].zero()
    out["release"].fill_bytes(0xFF)
    inb = _lib.SlotBatch(plane.ptr, None, S, steps)
    outb = _lib.OrderBatch(*(out[name].ptr for name in fslot.NAMES))
    reruns = ctypes.c_uint32()
    tier = {"run": None, "ladder": None, "lane": fslot.LANE, "scan": fslot.SCAN}[args.tier]
    run_flags = _lib.first_tier_flag(fslot.LANE) if args.tier == "ladder" else 0
    state = fd.DeviceBuffer(lib.fx_slot_state_bytes(steps, S)) if tier == fslot.SCAN else None

    def step():
        t1 = time.time()
        if tier is None:
            _lib.check(lib.fx_slot_run(ctypes.byref(inb), ctypes.byref(outb), run_flags, None, ctypes.byref(reruns)), "fx_slot_run")
        else:
            _lib.check(lib.fx_slot_execute(ctypes.byref(inb), ctypes.byref(outb), None, S, tier,
                                           state.ptr if state else None, 0, None), "fx_slot_execute")
        _lib.check(lib.fx_dev_synchronize(None), "sync")
        return 1e3 * (time.time() - t1)

    stages = []
    if args.kv:
        kv_ops = fd.synth_kv_ops(args.seed, S, steps, args.read_pct, args.delete_pct)
        kv_out = {"result": fd.DeviceBuffer(pw * 4), "store": fd.DeviceBuffer(S * args.keys * 4),
                  "monitor": fd.DeviceBuffer(pw * 4), "mon_off": fd.DeviceBuffer(S * (args.keys + 1) * 4),
                  "err": fd.DeviceBuffer(S * 4)}
        kv_in = _lib.KvBatch(out["order"].ptr, out["nexec"].ptr, plane.ptr, args.keys - 1, kv_ops.ptr, S, steps,
                             args.keys, 1)
        kv_outb = _lib.KvOut(*(kv_out[name].ptr for name in ("result", "store", "monitor", "mon_off", "err")))

        def kv_step():
            t1 = time.time()
            _lib.check(lib.fx_kv_execute(ctypes.byref(kv_in), ctypes.byref(kv_outb), None), "fx_kv_execute")
            _lib.check(lib.fx_dev_synchronize(None), "sync")
            return 1e3 * (time.time() - t1)
        stages.append(("kv_ms", kv_step, []))
    if args.pending:
        from fantoch_amd import pending as fp
        ones = fd.DeviceBuffer(pw * 4)
        ones.upload(np.ones(pw, np.uint32))
        pend_out = {name: fd.DeviceBuffer(words * 4)
                    for name, words in zip(fp.NAMES, (fp.MAX_PARTS * pw, pw, pw, pw, S, S, S))}
        pend_in = _lib.PendingBatch(out["order"].ptr, out["nexec"].ptr, plane.ptr, ones.ptr, 0xFFFFFFFF, 0, S, steps)
        pend_outb = _lib.PendingOut(*(pend_out[name].ptr for name in fp.NAMES))
        pend_reruns = ctypes.c_uint32()

        def pending_step():
            t1 = time.time()
            _lib.check(lib.fx_pending_run(ctypes.byref(pend_in), ctypes.byref(pend_outb), None,
                                          ctypes.byref(pend_reruns)), "fx_pending_run")
            _lib.check(lib.fx_dev_synchronize(None), "sync")
            return 1e3 * (time.time() - t1)
        stages.append(("pending_ms", pending_step, []))

    for _ in range(max(args.warmup, 1)):
        step()
        for _, fn, _ in stages:
            fn()
    ms = []
    for _ in range(args.steps):
        ms.append(step())
        for _, fn, times in stages:
            times.append(fn())

    nexec_h, err_h = out["nexec"].download(np.uint32, S), out["err"].download(np.uint32, S)
    rows, executed = S * steps, int(nexec_h.astype(np.uint64).sum())

    # parity sample: streams spread over the batch, their tiles downloaded
    tile_words = ((steps + 3) // 4) * 256

    def tile_of(buf, t, plane_no=0):
        a = np.empty(tile_words, np.uint32)
        _lib.check(lib.fx_dev_d2h(a.ctypes.data, buf.ptr + (plane_no * pw + t * tile_words) * 4, tile_words * 4, None),
                   "d2h")
        _lib.check(lib.fx_dev_synchronize(None), "sync")
        return a

    parity, checked = True, 0
    window = fslot.LANE_WINDOW if tier == fslot.LANE else None
    for j in range(args.sample):
        s = (j * 977 + 13) % S
        at = _lib.index(np.arange(steps), s % 64, steps)
        slots = [int(x) for x in tile_of(plane, s // 64)[at]]
        parity = parity and slots == fslot.synth_slot_streams_c6(args.seed, 1, steps, args.window, stream_base=s)[0]
        ref = slot_ref.run(slots, steps, window)
        o, r = tile_of(out["order"], s // 64)[at], tile_of(out["release"], s // 64)[at]
        want_r = np.full(steps, _lib.FX_RELEASE_NONE, np.uint32)
        for a, v in ref["release"].items():
            want_r[a] = v
        ok = (int(err_h[s]) == ref["err"] and int(nexec_h[s]) == ref["nexec"]
              and [int(x) & 0x7FFFFFFF for x in o[:ref["nexec"]]] == ref["order"] and np.array_equal(r, want_r))
        order = ref["order"]
        if args.kv and ok:
            import kv_ref
            want_res, want_store, want_mon = kv_ref.run(order, [k & (args.keys - 1) for k in slots],
                                                        [[int(w)] for w in tile_of(kv_ops, s // 64)[at]])
            res_rows, mon_rows = tile_of(kv_out["result"], s // 64)[at], tile_of(kv_out["monitor"], s // 64)[at]
            store = kv_out["store"].download(np.uint32, S * args.keys).reshape(S, args.keys)[s]
            off = kv_out["mon_off"].download(np.uint32, S * (args.keys + 1)).reshape(S, args.keys + 1)[s]
            ok = (all(int(res_rows[a]) == want_res[a][0] for a in order)
                  and store.tolist() == [want_store.get(k, 0) for k in range(args.keys)]
                  and all(mon_rows[int(off[k]):int(off[k + 1])].tolist() == want_mon.get(k, [])
                          for k in range(args.keys)))
        if args.pending and ok:
            import pending_ref
            want = pending_ref.run(order, slots, [1] * steps, steps)
            ready = tile_of(pend_out["ready"], s // 64)[at]
            ok = ready[:len(want["ready"])].tolist() == want["ready"] and \
                int(pend_out["nready"].download(np.uint32, S)[s]) == len(want["ready"])
        parity, checked = parity and ok, checked + 1

    step_ms = sum(ms) / len(ms)
    # one slot word read per row, one order word and one release word written per row
    alg_bytes = 12.0 * rows
    achieved = alg_bytes / (step_ms * 1e-3) / 1e9
    line = {
        "metric": "rows/sec, FPaxos SlotExecutor over batched streams (%s)" % (
            "fx_slot_run, LANE first" if args.tier == "ladder" else "fx_slot_run" if tier is None else "fx_slot_execute, %s tier" % args.tier),
        "value": round(rows / (step_ms * 1e-3), 1), "unit": "rows/s", "higher_is_better": True,
        "ms_per_step": round(step_ms, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
        "includes": "the call and a synchronise (wall clock); fx_slot_run also its status read-backs",
        "steps": args.steps, "warmup": args.warmup, "n_gpus": 1, "dtype": "u32",
        "tier": args.tier, "window": args.window, "reruns": int(reruns.value), "rerun_share": round(reruns.value / S, 4),
        "errors": int(np.count_nonzero(err_h)),
        "error_codes": {str(int(c)): int(np.count_nonzero(err_h == c)) for c in np.unique(err_h) if c},
        "rows_per_step": rows, "executed_per_step": executed,
        "config": {"streams": S, "slots_per_stream": steps, "seed": args.seed,
                   "parallelism": "LANE: a lane per stream, 64 streams per wavefront; SCAN: a wavefront per stream"},
        "roofline": {"bound": "hbm", "alg_bytes_per_step": int(alg_bytes),
                     "alg_bytes_definition": "12 B per row: one slot word read, one order word and one release word "
                                             "written",
                     "achieved_gbps": round(achieved, 3), "copy_gbps_same_session": round(copy, 1) if copy else None,
                     "frac_of_copy": round(achieved / copy, 5) if copy else None,
                     "peak": HBM_PEAK_GBPS, "frac_of_peak": round(achieved / HBM_PEAK_GBPS, 6)},
        "generation_ms": round(min(gen_ms[1:]), 3),
        "sample_parity": bool(parity), "sample_streams": checked,
    }
    for name, _, times in stages:
        line[name] = round(sum(times) / len(times), 3)
        line[name + "_min_max"] = [round(min(times), 3), round(max(times), 3)]
    if args.pending:
        line["pending_reruns"] = int(pend_reruns.value)
    if args.host:
        host = plane.download(np.uint32, pw)
        ho = {name: np.zeros(n, np.uint32) for name, n in zip(fslot.NAMES, (pw, pw, S, S))}
        tiles = (S + 63) // 64
        cuts = [tiles * i // args.threads for i in range(args.threads + 1)]

        def part(i):
            t0, t1 = cuts[i], cuts[i + 1]
            if t0 == t1:
                return 0
            n = min(S, t1 * 64) - t0 * 64
            b = _lib.SlotBatch(host.ctypes.data + t0 * tile_words * 4, None, n, steps)
            o = _lib.OrderBatch(ho["order"].ctypes.data + t0 * tile_words * 4,
                                ho["release"].ctypes.data + t0 * tile_words * 4, ho["nexec"].ctypes.data + t0 * 256,
                                ho["err"].ctypes.data + t0 * 256)
            return lib.fx_slot_execute_host(ctypes.byref(b), ctypes.byref(o), 0)

        with ThreadPoolExecutor(args.threads) as pool:
            t1 = time.time()
            sts = list(pool.map(part, range(args.threads)))
            line["host_ms"] = round(1e3 * (time.time() - t1), 3)
        line["host_threads"] = args.threads
        line["host_equals_device"] = bool(not any(sts) and tier != fslot.LANE and
                                          np.array_equal(ho["nexec"], nexec_h) and np.array_equal(ho["err"], err_h))
    print(json.dumps(line), flush=True)
    if args.record:
        path = os.path.join(ROOT, "profiles", "slot_bench.json")
        lines = json.load(open(path))["lines"] if os.path.exists(path) else []
        lines.append({"args": " ".join(sys.argv[1:]), "line": line})
        with open(path, "w") as f:
            json.dump({"what": "bench_slot.py lines, one per invocation (--record); ms_per_step is wall time around "
                               "the call and a synchronise, kv_ms and pending_ms are timed beside it", "lines": lines},
                      f, indent=1)
            f.write("\n")
    return 0 if parity else 1


if __name__ == "__main__":
    sys.exit(main())
