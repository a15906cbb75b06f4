"""The chain slot session -> KV session -> pending session on the GPU
(fx_slot_advance, fx_kv_advance, fx_pending_advance), against the whole stages.

Workload: bench_slot.py's chain: `--streams` streams of `--slots` slots each,
generated on the device (fx_slot_synth_generate), the slot plane as the key
plane (key = slot & (keys - 1)) and as the rifl plane, one generated op per row
(fx_kv_synth_ops) and a count plane of ones.  Nothing is uploaded per step.

One step feeds every stream in `--pieces` N equal pieces.  Three ways, step by
step in the same process on the same input buffers, in an order that alternates
from step to step:

  sessions  per piece fx_slot_advance, fx_kv_advance, fx_pending_advance (the
            first piece with FX_FLAG_INIT); one synchronise per step
            (`sessions_ms`), or one after every piece, as a caller that reads
            each piece's results does (`sessions_sync_ms`)
  whole     (a) fx_slot_run, fx_kv_execute, fx_pending_run once over the whole
            streams: the price of resumability at 1 piece
  rerun     (b) per piece fx_slot_advance, then fx_kv_execute and
            fx_pending_run over the session's cumulative order plane from row
            0: what a caller had to do before the stage sessions.
            fx_pending_run synchronises by itself, once per piece

Wall clock around the calls and the synchronise.  After the timed steps every
output of the sessions and of the reruns is compared with the whole chain's in
every word (the sessions' monitor through fx_kv_session_monitor), and a sample
of streams with tests/kv_ref.py and tests/pending_ref.py.  Prints one JSON line
and appends it to profiles/kv_session_bench.json with `--record`."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KV_NAMES = ("result", "store", "monitor", "mon_off", "err")


def stats(ms):
    return {"mean": round(sum(ms) / len(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=20480)
    ap.add_argument("--slots", type=int, default=1000)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--keys", type=int, default=16, help="a power of two")
    ap.add_argument("--read-pct", type=int, default=50)
    ap.add_argument("--delete-pct", type=int, default=10)
    ap.add_argument("--pieces", type=int, default=8)
    ap.add_argument("--sample", type=int, default=8)
    ap.add_argument("--record", action="store_true", help="append the line to profiles/kv_session_bench.json")
    args = ap.parse_args()
    if not 1 <= args.pieces <= max(args.slots, 1):
        raise SystemExit("--pieces must lie in 1 .. --slots")
    if args.keys & (args.keys - 1):
        raise SystemExit("--keys must be a power of two")

    from fantoch_amd import _lib
    from fantoch_amd import device as fd
    from fantoch_amd import pending as fp
    from fantoch_amd import slot as fslot
    import kv_ref
    import pending_ref
    lib = _lib.load()
    if lib.fx_device_count() <= 0:
        raise SystemExit("no GPU visible to libfantoch_amd")
    S, steps, N, keys = args.streams, args.slots, args.pieces, args.keys
    pw = _lib.plane_words(S, steps)
    check = _lib.check

    def sync():
        check(lib.fx_dev_synchronize(None), "sync")

    plane = fd.DeviceBuffer(pw * 4)
    check(lib.fx_slot_synth_generate(args.seed, 0, S, steps, None, args.window, plane.ptr, None), "generate")
    ops = fd.synth_kv_ops(args.seed, S, steps, args.read_pct, args.delete_pct)
    ones = fd.DeviceBuffer(pw * 4)
    ones.upload(np.ones(pw, np.uint32))
    cuts = [(steps * (i + 1) + N - 1) // N for i in range(N)]
    lengths = []
    for c in cuts:
        lengths.append(fd.DeviceBuffer(S * 4))
        lengths[-1].upload(np.full(S, c, np.uint32))

    def buffers(sizes):
        out = {name: fd.DeviceBuffer(n * 4) for name, n in sizes.items()}
        for b in out.values():
            b.zero()
        return out

    slot_sizes = dict(zip(fslot.NAMES, (pw, pw, S, S)))
    kv_sizes = dict(result=pw, store=S * keys, monitor=pw, mon_off=S * (keys + 1), err=S)
    pend_sizes = dict(zip(fp.NAMES, (fp.MAX_PARTS * pw, pw, pw, pw, S, S, S)))

    class Side:
        """The outputs of one contender, and the call structs over them."""

        def __init__(self, session_stages):
            self.slot, self.pend = buffers(slot_sizes), buffers(pend_sizes)
            self.kv = buffers(dict(kv_sizes, rank=pw) if session_stages else kv_sizes)
            self.slot_out = _lib.OrderBatch(*(self.slot[n].ptr for n in fslot.NAMES))
            self.kv_in = _lib.KvBatch(self.slot["order"].ptr, self.slot["nexec"].ptr, plane.ptr, keys - 1, ops.ptr, S,
                                      steps, keys, 1)
            self.kv_out = _lib.KvOut(*(self.kv[n].ptr for n in KV_NAMES))
            self.pend_in = _lib.PendingBatch(self.slot["order"].ptr, self.slot["nexec"].ptr, plane.ptr, ones.ptr,
                                             0xFFFFFFFF, 0, S, steps)
            self.pend_out = _lib.PendingOut(*(self.pend[n].ptr for n in fp.NAMES))
            self.slot_state = fd.DeviceBuffer(lib.fx_slot_session_bytes(steps, S))
            if session_stages:
                self.kv_ses_out = _lib.KvSessionOut(*(self.kv[n].ptr for n in ("result", "store", "rank", "err")))
                self.kv_state = fd.DeviceBuffer(lib.fx_kv_session_bytes(keys, S))
                self.pend_state = fd.DeviceBuffer(lib.fx_pending_session_bytes(steps, S))

        def get(self, group, name):
            buf = getattr(self, group)[name]
            return buf.download(np.uint32, buf.nbytes // 4)

    ses, whole, rerun = Side(True), Side(False), Side(False)
    piece_in = [_lib.SlotBatch(plane.ptr, l.ptr, S, steps) for l in lengths]
    whole_in = _lib.SlotBatch(plane.ptr, None, S, steps)
    reruns = ctypes.c_uint32()

    def sessions_step(sync_each):
        t1 = time.time()
        for i, b in enumerate(piece_in):
            init = _lib.FX_FLAG_INIT if i == 0 else 0
            check(lib.fx_slot_advance(ctypes.byref(b), ctypes.byref(ses.slot_out), ses.slot_state.ptr, init, None),
                  "fx_slot_advance")
            check(lib.fx_kv_advance(ctypes.byref(ses.kv_in), ctypes.byref(ses.kv_ses_out), ses.kv_state.ptr, init, None),
                  "fx_kv_advance")
            check(lib.fx_pending_advance(ctypes.byref(ses.pend_in), ctypes.byref(ses.pend_out), ses.pend_state.ptr, init,
                                         None), "fx_pending_advance")
            if sync_each:
                sync()
        sync()
        return 1e3 * (time.time() - t1)

    def whole_step():
        t1 = time.time()
        check(lib.fx_slot_run(ctypes.byref(whole_in), ctypes.byref(whole.slot_out), 0, None, None), "fx_slot_run")
        check(lib.fx_kv_execute(ctypes.byref(whole.kv_in), ctypes.byref(whole.kv_out), None), "fx_kv_execute")
        check(lib.fx_pending_run(ctypes.byref(whole.pend_in), ctypes.byref(whole.pend_out), None, ctypes.byref(reruns)),
              "fx_pending_run")
        sync()
        return 1e3 * (time.time() - t1)

    def rerun_step():
        t1 = time.time()
        for i, b in enumerate(piece_in):
            check(lib.fx_slot_advance(ctypes.byref(b), ctypes.byref(rerun.slot_out), rerun.slot_state.ptr,
                                      _lib.FX_FLAG_INIT if i == 0 else 0, None), "fx_slot_advance")
            check(lib.fx_kv_execute(ctypes.byref(rerun.kv_in), ctypes.byref(rerun.kv_out), None), "fx_kv_execute")
            check(lib.fx_pending_run(ctypes.byref(rerun.pend_in), ctypes.byref(rerun.pend_out), None,
                                     ctypes.byref(reruns)), "fx_pending_run")
        sync()
        return 1e3 * (time.time() - t1)

    contenders = [("sessions_ms", lambda: sessions_step(False)), ("sessions_sync_ms", lambda: sessions_step(True)),
                  ("whole_ms", whole_step), ("rerun_ms", rerun_step)]
    times = {name: [] for name, _ in contenders}
    for _ in range(max(args.warmup, 1)):
        for _, fn in contenders:
            fn()
    for k in range(args.steps):
        for name, fn in (contenders if k % 2 == 0 else contenders[::-1]):
            times[name].append(fn())

    # every timed output against the whole chain's; the sessions' monitor is built on demand
    check(lib.fx_kv_session_monitor(ctypes.byref(ses.kv_in), ses.kv["rank"].ptr, ctypes.byref(ses.kv_out),
                                    ses.kv_state.ptr, None), "fx_kv_session_monitor")
    sync()
    differ = {"sessions": [], "rerun": []}
    for group, names in (("slot", fslot.NAMES), ("kv", KV_NAMES), ("pend", fp.NAMES)):
        for n in names:  # one buffer of each side at a time
            want = whole.get(group, n)
            for who, side in (("sessions", ses), ("rerun", rerun)):
                if not np.array_equal(side.get(group, n), want):
                    differ[who].append(group + "." + n)
    equal = not differ["sessions"] and not differ["rerun"]
    got = {(g, n): ses.get(g, n) for g, n in (("slot", "order"), ("slot", "nexec"), ("slot", "err"), ("kv", "result"),
                                               ("kv", "store"), ("kv", "monitor"), ("kv", "mon_off"), ("kv", "err"),
                                               ("pend", "ready"), ("pend", "nready"), ("pend", "err"))}

    host_plane, host_ops = plane.download(np.uint32, pw), ops.download(np.uint32, pw)
    parity, checked = True, 0
    for j in range(args.sample):
        s = (j * 977 + 13) % S
        at = _lib.index(np.arange(steps), s, steps)
        slots = [int(x) for x in host_plane[at]]
        ne = int(got[("slot", "nexec")][s])
        order = [int(x) & 0x7FFFFFFF for x in got[("slot", "order")][at][:ne]]
        want_res, want_store, want_mon = kv_ref.run(order, [k & (keys - 1) for k in slots],
                                                    [[int(w)] for w in host_ops[at]])
        off = got[("kv", "mon_off")].reshape(S, keys + 1)[s]
        mon = got[("kv", "monitor")][at]
        ok = (all(int(got[("kv", "result")][at][a]) == want_res[a][0] for a in order)
              and got[("kv", "store")].reshape(S, keys)[s].tolist() == [want_store.get(k, 0) for k in range(keys)]
              and all(mon[int(off[k]):int(off[k + 1])].tolist() == want_mon.get(k, []) for k in range(keys)))
        ref = pending_ref.run(order, slots, [1] * steps, steps)
        ok = ok and got[("pend", "ready")][at][:len(ref["ready"])].tolist() == ref["ready"] and \
            int(got[("pend", "nready")][s]) == len(ref["ready"]) and ne == steps
        parity, checked = parity and ok, checked + 1

    rows = S * steps
    mean = {name: sum(t) / len(t) for name, t in times.items()}
    line = {
        "metric": "rows/sec, slot session + KV session + pending session (%d pieces per step)" % N,
        "value": round(rows / (mean["sessions_ms"] * 1e-3), 1), "unit": "rows/s", "higher_is_better": True,
        "pieces": N, "rows_per_piece": cuts[0], "steps": args.steps, "warmup": args.warmup, "n_gpus": 1, "dtype": "u32",
        "includes": "wall clock around the calls of a step and the synchronise; the contenders run step by step in "
                    "turn, in an order that alternates",
        "sessions_ms": stats(times["sessions_ms"]), "sessions_sync_ms": stats(times["sessions_sync_ms"]),
        "whole_ms": stats(times["whole_ms"]), "rerun_ms": stats(times["rerun_ms"]),
        "ratio_sessions_to_whole": round(mean["sessions_ms"] / mean["whole_ms"], 3),
        "ratio_sessions_to_rerun": round(mean["sessions_ms"] / mean["rerun_ms"], 3),
        "ratio_sessions_sync_to_rerun": round(mean["sessions_sync_ms"] / mean["rerun_ms"], 3),
        "rerun_rows_factor": round(sum(cuts) / steps, 3),
        "config": {"streams": S, "slots_per_stream": steps, "keys": keys, "window": args.window, "seed": args.seed,
                   "read_pct": args.read_pct, "delete_pct": args.delete_pct,
                   "parallelism": "a wavefront per stream and call"},
        "equals_whole_chain": bool(equal), "differing": differ, "sample_parity": bool(parity), "sample_streams": checked,
        "errors": int(sum(np.count_nonzero(got[(g, "err")]) for g in ("slot", "kv", "pend"))),
    }
    print(json.dumps(line), flush=True)
    if args.record:
        path = os.path.join(ROOT, "profiles", "kv_session_bench.json")
        lines = json.load(open(path))["lines"] if os.path.exists(path) else []
        lines.append({"args": " ".join(sys.argv[1:]), "line": line})
        with open(path, "w") as f:
            json.dump({"what": "bench_kv_session.py lines, one per invocation (--record): wall time per step (mean, "
                               "min, max over the steps) of the stage sessions, of the whole stages once and of the "
                               "whole stages rerun after every piece, step by step in turn in the same process",
                       "lines": lines}, f, indent=1)
            f.write("\n")
    return 0 if parity and equal else 1


if __name__ == "__main__":
    sys.exit(main())
