"""bench_pred_session.py: sessions of the predecessors executor
(fx_pred_advance) against whole runs (fx_pred_execute), in one process.

Streams: those of `bench.py --mode pred` at its default shape (fx_synth's
EPaxos-shaped commit streams, n = 5, 4096 seeds x conflicts 0,2,10,50,100,
1000 commands per process, the Caesar clock (seq, process id) of each dot),
generated on the device.  Lines, each timed with device events around the
calls of a step and one synchronise behind them:
  whole SMALL       one fx_pred_execute at SMALL over every stream
  session SMALL/N   N fx_pred_advance calls at SMALL, piece i = rows
                    [i steps / N, (i + 1) steps / N) of every stream, the
                    first with FX_FLAG_INIT; N = 1, 8, 64
  session LDS/N     the same at the LDS tier
Every line is warmed up, then timed until it has 20 steps or one second (three
steps at least).  After the last piece of every session line every output word
is compared with the whole run at that tier and, on the first 64 streams, with
the host twin fed the same pieces; the streams that stop with FX_ERR_CAPACITY
at SMALL are counted in both and must be as many.  The CPU column is the twin
(fx_pred_advance_host, up to 16 threads) over the first --cpu-streams streams
in one piece.  Prints one JSON line and, with --record, writes
profiles/pred_resume_bench.json."""
import argparse
import ctypes
import json
import os
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=4096)
    ap.add_argument("--conflicts", type=str, default="0,2,10,50,100")
    ap.add_argument("--cmds", type=int, default=1000)
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--cycle-pct", type=int, default=30)
    ap.add_argument("--seed", type=int, default=20250213)
    ap.add_argument("--pieces", type=str, default="1,8,64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--cpu-streams", type=int, default=1024)
    ap.add_argument("--record", action="store_true")
    args = ap.parse_args()

    import torch

    from fantoch_amd import _lib
    from fantoch_amd import streams as fs

    lib = _lib.load()
    if lib.fx_device_count() <= 0:
        raise SystemExit("no GPU visible to libfantoch_amd")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    conflicts = tuple(int(c) for c in args.conflicts.split(","))
    pieces = [int(x) for x in args.pieces.split(",")]
    p = fs.synth_params(seed=args.seed, instances=args.seeds * len(conflicts), n=args.n, cmds=args.cmds,
                        window=args.window, cycle_pct=args.cycle_pct, conflicts=conflicts, conflict_block=args.seeds)
    S, steps, dmax = fs.synth_shape(p)
    pw = _lib.plane_words(S, steps)
    hs = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    SMALL, LDS = _lib.FX_PRED_TIER_SMALL, _lib.FX_PRED_TIER_LDS
    CAPACITY = _lib.FX_ERR_CAPACITY

    def buf(words):
        return torch.zeros(words, dtype=torch.int32, device=dev)

    dot, hdr, deps = buf(pw), buf(pw), buf(pw * dmax)
    _lib.check(lib.fx_synth_generate(ctypes.byref(p), dot.data_ptr(), hdr.data_ptr(), deps.data_ptr(), hs),
               "fx_synth_generate")
    clo = (((dot & 0xFFFFFF) << 8) | ((dot >> 24) & 0xFF)).contiguous()
    chi = torch.zeros_like(clo)
    torch.cuda.synchronize(dev)

    class Outputs:
        def __init__(self):
            self.t = [buf(pw), buf(pw), buf(S), buf(S)]
            self.b = _lib.OrderBatch(*[x.data_ptr() for x in self.t])

        def same(self, other):
            return all(bool(torch.equal(a, b)) for a, b in zip(self.t, other.t))

        def capacity(self):
            return int((self.t[3] == CAPACITY).sum().item())

    def batch(lengths):
        base = _lib.StreamBatch(dot.data_ptr(), hdr.data_ptr(), deps.data_ptr(), lengths, S, steps, dmax, args.n)
        return _lib.PredBatch(base, clo.data_ptr(), chi.data_ptr(), None)

    def timed(step):
        """Warm-up, then steps until args.steps of them or args.seconds (three at least): ms per step."""
        step()
        torch.cuda.synchronize(dev)
        ms, t0 = [], time.time()
        while len(ms) < 3 or (len(ms) < args.steps and time.time() - t0 < args.seconds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            torch.cuda.synchronize(dev)
            ms.append(e0.elapsed_time(e1))
        return {"ms_per_step": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                "timed_steps": len(ms)}

    lines, whole = [], {}
    for tier in (SMALL, LDS):
        out = Outputs()
        inb = batch(None)

        def step(tier=tier, out=out, inb=inb):
            _lib.check(lib.fx_pred_execute(ctypes.byref(inb), ctypes.byref(out.b), None, S, tier, None, 0, hs),
                       "fx_pred_execute")
        line = dict(name="whole %s" % ("SMALL" if tier == SMALL else "LDS"), tier=tier, pieces=0, **timed(step))
        whole[tier] = (out, line["ms_per_step"])
        if tier == SMALL:
            lines.append(line)
        else:
            line["note"] = "beside the issue's lines: what the LDS sessions are compared with"
            lines.append(line)
    executed = int(whole[SMALL][0].t[2].to(torch.int64).sum().item())

    # the first tile of every plane: streams 0 .. 63, a contiguous prefix
    Ss = min(S, 64)
    tw = _lib.plane_words(Ss, steps)

    def pre(t, k=1):
        return np.ascontiguousarray(t.view(k, pw)[:, :tw].cpu().numpy().view(np.uint32).reshape(-1))
    h_dot, h_hdr, h_deps, h_clo, h_chi = pre(dot), pre(hdr), pre(deps, dmax), pre(clo), pre(chi)

    def twin(tier, cuts, streams=Ss, planes=None):
        """The host twin over the first `streams` streams, fed the pieces `cuts`: (outputs, seconds)."""
        d, h, dp, cl, ch = planes or (h_dot, h_hdr, h_deps, h_clo, h_chi)
        w = _lib.plane_words(streams, steps)
        outs = [np.zeros(k, np.uint32) for k in (w, w, streams, streams)]
        state = np.zeros(lib.fx_pred_session_bytes(tier, args.n, dmax, streams), np.uint8)
        outb = _lib.OrderBatch(*[a.ctypes.data for a in outs])
        t0 = time.time()
        for i, c in enumerate(cuts):
            lens = np.full(streams, c, np.uint32)
            base = _lib.StreamBatch(d.ctypes.data, h.ctypes.data, dp.ctypes.data, lens.ctypes.data, streams, steps,
                                    dmax, args.n)
            inb = _lib.PredBatch(base, cl.ctypes.data, ch.ctypes.data, None)
            _lib.check(lib.fx_pred_advance_host(ctypes.byref(inb), ctypes.byref(outb), tier, state.ctypes.data,
                                                _lib.FX_FLAG_INIT if i == 0 else 0), "fx_pred_advance_host")
        return outs, time.time() - t0

    for tier in (SMALL, LDS):
        state = torch.zeros(lib.fx_pred_session_bytes(tier, args.n, dmax, S) // 4, dtype=torch.int32, device=dev)
        for N in pieces:
            cuts = [steps * (i + 1) // N for i in range(N)]
            lens = [torch.full((S,), c, dtype=torch.int32, device=dev) for c in cuts]
            calls = [batch(x.data_ptr()) for x in lens]
            out = Outputs()

            def step(tier=tier, out=out, calls=calls, state=state):
                for i, inb in enumerate(calls):
                    _lib.check(lib.fx_pred_advance(ctypes.byref(inb), ctypes.byref(out.b), tier, state.data_ptr(),
                                                   _lib.FX_FLAG_INIT if i == 0 else 0, hs), "fx_pred_advance")
            line = dict(name="session %s/%d" % ("SMALL" if tier == SMALL else "LDS", N), tier=tier, pieces=N,
                        rows_per_piece=cuts[0], **timed(step))
            ref, ref_ms = whole[tier]
            line["vs_whole_same_tier"] = round(line["ms_per_step"] / ref_ms, 3)
            line["vs_whole_small"] = round(line["ms_per_step"] / whole[SMALL][1], 3)
            line["parity_whole"] = out.same(ref)
            t_outs, _ = twin(tier, cuts)
            line["parity_twin_64"] = all(np.array_equal(a, b) for a, b in zip(
                t_outs, (pre(out.t[0]), pre(out.t[1]), out.t[2][:Ss].cpu().numpy().view(np.uint32),
                         out.t[3][:Ss].cpu().numpy().view(np.uint32))))
            if tier == SMALL:
                line["capacity_streams"] = {"whole": ref.capacity(), "session": out.capacity()}
                line["parity_capacity"] = ref.capacity() == out.capacity()
            lines.append(line)
            del out, lens, calls
        del state

    # the CPU column: the twin over the first tiles, one piece
    Sc = min(S, max(64, args.cpu_streams // 64 * 64))
    cw = _lib.plane_words(Sc, steps)

    def prec(t, k=1):
        return np.ascontiguousarray(t.view(k, pw)[:, :cw].cpu().numpy().view(np.uint32).reshape(-1))
    c_outs, c_dt = twin(SMALL, [steps], Sc, (prec(dot), prec(hdr), prec(deps, dmax), prec(clo), prec(chi)))
    cpu = {"streams": Sc, "adds": Sc * steps, "seconds": round(c_dt, 3), "threads": min(16, os.cpu_count() or 1),
           "adds_per_second": round(Sc * steps / c_dt, 1),
           "ms_per_step_scaled_to_the_batch": round(c_dt * 1e3 * S / Sc, 1),
           "parity_device": bool(np.array_equal(c_outs[2], whole[SMALL][0].t[2][:Sc].cpu().numpy().view(np.uint32)))}
    result = {
        "what": "fx_pred_advance sessions against fx_pred_execute whole, bench.py --mode pred's default streams, "
                "one process; ms_per_step = median of device-event times around the calls of a step",
        "config": {"streams": S, "adds_per_stream": steps, "n": args.n, "dmax": dmax, "seeds": args.seeds,
                   "conflicts": list(conflicts), "cmds": args.cmds, "adds": S * steps,
                   "executed_whole_small": executed},
        "session_bytes_per_stream": {"SMALL": lib.fx_pred_session_bytes(SMALL, args.n, dmax, 1),
                                     "LDS": lib.fx_pred_session_bytes(LDS, args.n, dmax, 1)},
        "lines": lines, "cpu": cpu,
        "parity": all(l.get("parity_whole", True) and l.get("parity_twin_64", True) and l.get("parity_capacity", True)
                      for l in lines) and cpu["parity_device"],
    }
    print(json.dumps(result), flush=True)
    if args.record:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "pred_resume_bench.json")
        with open(path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0 if result["parity"] else 1


if __name__ == "__main__":
    raise SystemExit(main())
