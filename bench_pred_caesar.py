"""bench_pred_caesar.py: the predecessors executor (fx_pred_run) over streams
in the shape of Caesar's own commits, generated on the device
(fx_pred_synth_generate; the model is csrc/fx_pred_synth.h), in one process.

Default batch: 4,096 instances of n = 5 with 200 commands per process,
conflicts 2 / 10 / 50 / 100 % in blocks of 1,024 instances, window 8, horizon
4, max_bump 2, retry 30 %: 20,480 streams of 1,000 Adds, dmax = 34.  Lines,
each timed with device events around the call and one synchronise behind it,
warmed up, then until --steps of them or --seconds (three at least):
  generate tile / command   the two forms of the generator's kernel
  run caesar                fx_pred_run over the generated batch
  run epaxos                fx_pred_run over the fx_synth batch of equal size
                            (bench.py --mode pred's streams: one dep per
                            source, the clock of each dot)
Beside them: mean and maximum deps per Add, the share of deps that wait for
the commit alone (the dep's final clock is the higher one), the streams that
ran again at each tier, and the first 64 streams checked against the oracle
(oracle_lib.pred_batch_execute with the ndeps plane).  Prints one JSON line
and, with --record, writes profiles/pred_caesar_bench.json."""
import argparse
import ctypes
import json
import os
import time
import types

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--conflicts", type=str, default="2,10,50,100")
    ap.add_argument("--cmds", type=int, default=200)
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=4)
    ap.add_argument("--max-bump", type=int, default=2)
    ap.add_argument("--retry-pct", type=int, default=30)
    ap.add_argument("--seed", type=int, default=20250213)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--record", action="store_true")
    args = ap.parse_args()

    import torch

    from fantoch_amd import _lib
    from fantoch_amd import pred as fpred
    from fantoch_amd import streams as fs
    from oracle import oracle_lib

    lib = _lib.load()
    if lib.fx_device_count() <= 0:
        raise SystemExit("no GPU visible to libfantoch_amd")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    hs = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    conflicts = tuple(int(c) for c in args.conflicts.split(","))
    block = max(args.instances // len(conflicts), 1)
    p = fpred.pred_synth_params(seed=args.seed, instances=args.instances, n=args.n, cmds=args.cmds, window=args.window,
                                horizon=args.horizon, max_bump=args.max_bump, retry_pct=args.retry_pct,
                                conflicts=conflicts, conflict_block=block)
    S, steps, dmax = fpred.pred_synth_shape(p)
    n = args.n
    pw = _lib.plane_words(S, steps)
    SMALL, LDS, HBM = _lib.FX_PRED_TIER_SMALL, _lib.FX_PRED_TIER_LDS, _lib.FX_PRED_TIER_HBM

    def buf(words):
        return torch.zeros(words, dtype=torch.int32, device=dev)

    def timed(step):
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

    # ---------------------------------------------------------------- generation, both forms
    dot, hdr, clo, chi, nd, deps = buf(pw), buf(pw), buf(pw), buf(pw), buf(pw), buf(pw * max(dmax, 1))
    planes = _lib.PredSynthPlanes(dot.data_ptr(), hdr.data_ptr(), deps.data_ptr(), clo.data_ptr(), chi.data_ptr(),
                                  nd.data_ptr())
    gen = {}
    for name, form in (("command", _lib.FX_PRED_SYNTH_FORM_COMMAND), ("tile", _lib.FX_PRED_SYNTH_FORM_TILE)):
        def step(form=form):
            _lib.check(lib.fx_pred_synth_generate_form(ctypes.byref(p), ctypes.byref(planes), form, hs),
                       "fx_pred_synth_generate_form")
        gen[name] = timed(step)
    _lib.check(lib.fx_pred_synth_generate(ctypes.byref(p), ctypes.byref(planes), hs), "fx_pred_synth_generate")
    torch.cuda.synchronize(dev)
    words = S * steps * (dmax + 5)
    for g in gen.values():
        g["written_gb_per_s"] = round(words * 4 / (g["ms_per_step"] * 1e-3) / 1e9, 1)

    # ---------------------------------------------------------------- the batch's deps
    pos = torch.arange(pw, device=dev, dtype=torch.int64)
    steps4 = (steps + 3) // 4
    tile = pos // 256
    stream = (tile // steps4) * 64 + (pos % 256) // 4
    row = (tile % steps4) * 4 + pos % 4
    valid = (stream < S) & (row < steps)
    del pos, tile, row
    clock = ((chi.to(torch.int64) & 0xFFFFFFFF) << 32) | (clo.to(torch.int64) & 0xFFFFFFFF)

    def command_of(d):  # g of a packed dot
        d = d.to(torch.int64)
        return ((d & 0xFFFFFF) - 1) * n + ((d >> 24) & 0xFF) - 1
    table = torch.zeros(S * steps, dtype=torch.int64, device=dev)  # final clock by (stream, g)
    table[(stream * steps + command_of(dot))[valid]] = clock[valid]
    ndv = nd[valid].to(torch.int64)
    dep_total, dep_max = int(ndv.sum().item()), int(ndv.max().item())
    commit_only, has, c2 = 0, None, None
    for k in range(dmax):
        has = valid & (nd > k)
        c2 = table[(stream * steps + command_of(deps[k * pw:(k + 1) * pw]))[has]]
        commit_only += int((c2 > clock[has]).sum().item())
    del table, stream, valid, clock, ndv, has, c2

    # ---------------------------------------------------------------- fx_pred_run
    order, release, nexec, err = buf(pw), buf(pw), buf(S), buf(S)
    outb = _lib.OrderBatch(order.data_ptr(), release.data_ptr(), nexec.data_ptr(), err.data_ptr())
    base = _lib.StreamBatch(dot.data_ptr(), hdr.data_ptr(), deps.data_ptr(), None, S, steps, dmax, n)
    inb = _lib.PredBatch(base, clo.data_ptr(), chi.data_ptr(), nd.data_ptr())
    reruns = ctypes.c_uint32()

    def run(inb=inb):
        _lib.check(lib.fx_pred_run(ctypes.byref(inb), ctypes.byref(outb), 0, hs, ctypes.byref(reruns)), "fx_pred_run")
    caesar = timed(run)
    caesar["reruns"] = int(reruns.value)
    executed = int(nexec.to(torch.int64).sum().item())
    errors = int((err != 0).sum().item())
    caesar["adds_per_second"] = round(executed / (caesar["ms_per_step"] * 1e-3), 1)

    # the first 64 streams against the oracle
    Ss = min(S, 64)
    tw = _lib.plane_words(Ss, steps)

    def pre(t, k=1):
        return np.ascontiguousarray(t.view(k, pw)[:, :tw].cpu().numpy().view(np.uint32).reshape(-1))
    hp = types.SimpleNamespace(dot=pre(dot), hdr=pre(hdr), deps=pre(deps, max(dmax, 1)), lengths=None, S=Ss,
                               steps=steps, dmax=dmax, n=n, plane=tw)
    o_order, o_rel, o_nexec, o_err = oracle_lib.pred_batch_execute(hp, pre(clo), pre(chi), threads=min(16, os.cpu_count() or 1),
                                                                   ndeps=pre(nd))
    g_order, g_rel = pre(order), pre(release)
    parity = bool(np.array_equal(o_nexec, nexec[:Ss].cpu().numpy().view(np.uint32)) and not o_err.any() and
                  not err[:Ss].any().item())
    for s in range(Ss):
        rows = _lib.index(np.arange(int(o_nexec[s])), s, steps)
        allr = _lib.index(np.arange(steps), s, steps)
        parity = parity and bool(np.array_equal(g_order[rows], o_order[rows]) and np.array_equal(g_rel[allr], o_rel[allr]))

    # the streams that run again at each tier (one launch per tier, not timed)
    CAPACITY = _lib.FX_ERR_CAPACITY
    tiers = {}
    st = lib.fx_pred_execute(ctypes.byref(inb), ctypes.byref(outb), None, S, SMALL, None, 0, hs)
    torch.cuda.synchronize(dev)
    if st == _lib.FX_ERR_UNSUPPORTED:
        tiers["SMALL"], again = "the tables do not fit", torch.arange(S, dtype=torch.int32, device=dev)
    else:
        _lib.check(st, "fx_pred_execute SMALL")
        again = torch.nonzero(err == CAPACITY).reshape(-1).to(torch.int32).contiguous()
        tiers["SMALL"] = {"streams": S, "out_of_capacity": int(again.numel())}
    if again.numel():
        st = lib.fx_pred_execute(ctypes.byref(inb), ctypes.byref(outb), again.data_ptr(), int(again.numel()), LDS, None,
                                 0, hs)
        torch.cuda.synchronize(dev)
        if st == _lib.FX_ERR_UNSUPPORTED:
            tiers["LDS"] = "the tables do not fit"
            tiers["HBM"] = {"streams": int(again.numel())}
        else:
            _lib.check(st, "fx_pred_execute LDS")
            left = int((err == CAPACITY).sum().item())
            tiers["LDS"] = {"streams": int(again.numel()), "out_of_capacity": left}
            tiers["HBM"] = {"streams": left}
    del order, release

    # ---------------------------------------------------------------- the EPaxos-shaped batch of equal size
    q = fs.synth_params(seed=args.seed, instances=args.instances, n=n, cmds=args.cmds, window=args.window, cycle_pct=30,
                        conflicts=conflicts, conflict_block=block)
    S2, steps2, dmax2 = fs.synth_shape(q)
    assert (S2, steps2) == (S, steps)
    e_dot, e_hdr, e_deps = buf(pw), buf(pw), buf(pw * dmax2)
    _lib.check(lib.fx_synth_generate(ctypes.byref(q), e_dot.data_ptr(), e_hdr.data_ptr(), e_deps.data_ptr(), hs),
               "fx_synth_generate")
    e_clo = (((e_dot & 0xFFFFFF) << 8) | ((e_dot >> 24) & 0xFF)).contiguous()
    e_chi = torch.zeros_like(e_clo)
    torch.cuda.synchronize(dev)
    order, release = buf(pw), buf(pw)
    outb = _lib.OrderBatch(order.data_ptr(), release.data_ptr(), nexec.data_ptr(), err.data_ptr())
    e_base = _lib.StreamBatch(e_dot.data_ptr(), e_hdr.data_ptr(), e_deps.data_ptr(), None, S, steps, dmax2, n)
    e_inb = _lib.PredBatch(e_base, e_clo.data_ptr(), e_chi.data_ptr(), None)
    epaxos = timed(lambda: run(e_inb))
    epaxos["reruns"] = int(reruns.value)
    e_executed = int(nexec.to(torch.int64).sum().item())
    epaxos["adds_per_second"] = round(e_executed / (epaxos["ms_per_step"] * 1e-3), 1)
    epaxos["mean_deps_per_add"] = round(float(((e_hdr.to(torch.int64) >> 24) & 31).sum().item()) / (S * steps), 3)
    epaxos["dmax"] = dmax2

    result = {
        "what": "fx_pred_run over device-generated Caesar commit streams (fx_pred_synth_generate), and over the "
                "fx_synth batch of equal size, one process; ms_per_step = median of device-event times",
        "config": {"streams": S, "adds_per_stream": steps, "adds": S * steps, "n": n, "dmax": dmax,
                   "instances": args.instances, "conflicts": list(conflicts), "conflict_block": block,
                   "cmds": args.cmds, "window": args.window, "horizon": args.horizon, "max_bump": args.max_bump,
                   "retry_pct": args.retry_pct, "dep_plane_bytes": pw * 4 * dmax, "words_written": words},
        "generate": gen,
        "deps": {"mean_per_add": round(dep_total / (S * steps), 3), "max_per_add": dep_max,
                 "commit_only_share": round(commit_only / max(dep_total, 1), 4)},
        "run_caesar": caesar, "executed": executed, "streams_with_errors": errors, "tiers": tiers,
        "run_epaxos_shaped": epaxos,
        "caesar_over_epaxos_step_time": round(caesar["ms_per_step"] / epaxos["ms_per_step"], 3),
        "parity_oracle_64": parity,
    }
    result["ok"] = bool(parity and errors == 0 and executed == S * steps)
    print(json.dumps(result), flush=True)
    if args.record:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "pred_caesar_bench.json")
        with open(path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0 if result["ok"] else 1


if __name__ == "__main__":
    raise SystemExit(main())
