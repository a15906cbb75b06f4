"""Tempo's TableExecutor on the GPU over batched streams (fx_table_run).

Workload: `--streams` streams per conflict rate in `--conflicts`, n = 5,
f = 1 (fast quorum 3, stability threshold 3), `--cmds` single-key commands
each over `--keys` keys, detached votes up to `--lag` and commits up to
`--window` commands late (fantoch_amd.table.synth_table_streams).  The
generator is plain Python, so `--distinct` streams (a multiple of 64: whole
plane tiles) are generated per conflict rate and each tile is laid out
streams / distinct times; every copy is its own memory and its own wavefront.

One step = fx_table_run over every stream (ONCHIP tier, capacity reruns on
HBM).  The ONCHIP kernel is timed by HIP events on its stream
(fx_profile_slot_ms); a sample of streams is then checked bit for bit against
the CPU restatement (tests/table_ref.py).  Prints one JSON line.

`--kmax K` (K > 1) is the multi-key line: commands of 1..K keys
(fantoch_amd.table.synth_table_streams_mk) through fx_table_run_mk, checked
against tests/table_ref_mk.py.

`--shards G` (G > 1) is the line of commands that span shards: groups of G
shard executors co-simulated on the CPU (tests/table_shapes_ps.py
synth_table_group: `--cmds` commands per shard executor on average, 1..G
shards and 1..kmax keys on each per command, StableAtShard messages up to
`--msg-lag` rounds late), every shard's stream through fx_table_run_ps,
checked against tests/table_ref_ps.py, stable_sent included.

`--chunks C` (C > 0) measures resumable streams instead: one step = every
stream on the HBM tier through C fx_table_advance calls, each handing the
executor the next 1/C of every stream (the first with FX_FLAG_INIT); the line
then also carries the time of the same streams whole through one
fx_table_execute* launch at the HBM tier and the state bytes a call reads and
writes.

`--device-synth` generates the streams on the device instead
(fx_table_synth_generate; fantoch_amd.device.DeviceTable): every stream of
the launch is distinct (`--distinct` is not used), nothing is uploaded, and
the line gains generation_ms, both passes of the generator timed around a
synchronise.  The sampled streams are downloaded tile by tile, compared with
the Python restatement of the generator
(fantoch_amd.table.synth_table_streams_c6) and run through the CPU
restatement of the executor.  Not with `--shards` alone: the host-paced
streams of a group hold the StableAtShard messages, which depend on the
executors' own stable_sent; a group's own events do not, see below.

`--shards G --in-kernel` (G of 2, 4 or 8) runs the same groups with the
closed loop inside the kernel: only the own events of synth_table_group's
streams go in, laid out as above, and one step = one fx_table_run_groups over
every group (one workgroup per group; a message is late by a hash of itself
in 0..`--msg-lag` rounds).  A sample of groups is checked against the closed
loop restated on the CPU (tests/table_resume.py closed_loop): the streams as
handled and every result.  The line reports the streams that
stopped with an error and the highest number of rounds.

`--device-synth --shards G --in-kernel` generates the groups on the device
(fx_table_group_synth_generate; fantoch_amd.device.DeviceTableGroups): every
group of the launch is distinct, nothing is uploaded, the delays are the
generator's own draws in 0..`--msg-lag`, and the line gains generation_ms as
above.  The sampled groups are downloaded and compared with the Python
restatement of the generator (fantoch_amd.table.synth_table_groups_c6) packed
by pack_table_groups -- streams, route and target lists -- before their
results are compared with closed_loop over them; the line also counts the
attached events of the sampled streams that stay unexecuted
(sample_attached_not_executed).

`--kv [--read-pct P] [--delete-pct D]` (the single-key and `--kmax` lines,
host- or device-generated streams) adds the KV stage: after each executor step
one fx_kv_execute over the step's own order plane and nexec, the hdr plane as
the key plane, and one op per row generated on the device (fx_kv_synth_ops: P
percent GETs, D percent DELETEs, PUTs otherwise).  The line gains kv_ms (wall
time around the launch and a synchronise, as generation_ms; it is not part of
ms_per_step or of the events/s value) and the pass's algorithmic bytes, and the
sampled streams' results, stores and monitors are checked against the
restatement of kvs.rs and monitor.rs (tests/kv_ref.py).

`--pending` (with `--kmax` above 1; host- or device-generated streams, with or
without `--kv`, `--shards` and `--in-kernel`, not with `--chunks`) adds the
pending stage: after each executor step (and the KV stage) one fx_pending_run
over the step's own order plane and nexec, the dot plane as the rifl plane and
the nkeys plane as the count plane.  With `--in-kernel` the order names handled
rows: their rifl and count planes are gathered once, before the timed steps,
through handled_src and handled_dot (every step handles the same input).  The line gains pending_ms (timed as kv_ms
and likewise outside ms_per_step), nready, nopen and the share of streams rerun
on the HBM tier; the sampled streams' heads, parts and ready lists are checked
against the restatement of aggregate.rs (tests/pending_ref.py), and the record
is also written to profiles/table_pending_bench.json."""
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

HBM_PEAK_GBPS = 8000.0


def pending_setup(fd, _lib, order, nexec, rifl, count, count_mask, S, steps):
    """The buffers and the timed call of the pending stage over one order plane: (outputs by name, step())."""
    from fantoch_amd import pending as fp
    lib = _lib.load()
    pw = _lib.plane_words(S, steps)
    out = {name: fd.DeviceBuffer(words * 4) for name, words in zip(fp.NAMES, (fp.MAX_PARTS * pw, pw, pw, pw, S, S, S))}
    inb = _lib.PendingBatch(order.ptr, nexec.ptr, rifl.ptr, count.ptr, count_mask, 0, S, steps)
    outb = _lib.PendingOut(*(out[name].ptr for name in fp.NAMES))
    reruns = ctypes.c_uint32()

    def step():
        t1 = time.time()
        _lib.check(lib.fx_pending_run(ctypes.byref(inb), ctypes.byref(outb), None, ctypes.byref(reruns)),
                   "fx_pending_run")
        _lib.check(lib.fx_dev_synchronize(None), "sync")
        return 1e3 * (time.time() - t1)

    return out, step, reruns


def pending_sample_ok(want, pend_h, s, head_rows, ready_rows, part_rows):
    """One sampled stream's heads, parts and ready list against the restatement's."""
    return (int(pend_h["err"][s]) == want["err"] == 0 and int(pend_h["nopen"][s]) == want["nopen"]
            and int(pend_h["nready"][s]) == len(want["ready"])
            and ready_rows[:len(want["ready"])].tolist() == want["ready"]
            and all(int(head_rows[a]) == h for a, h in want["head"].items())
            and all(int(part_rows[j][h]) == a for (j, h), a in want["part"].items()))


def pending_report(line, pending_ms, pend_h, reruns, S, executed, peak_live):
    """pending_ms and the stage's figures into the line, and the record into profiles/table_pending_bench.json."""
    # per executed row the order, rifl and count words read and the head and part words written (20 B), per
    # completed command an index and a ready word; per stream nexec read, nready, nopen and err written
    nready = int(pend_h["nready"].astype(np.uint64).sum())
    pend_bytes = 20.0 * executed + 8.0 * nready + 16.0 * S
    pend_avg = sum(pending_ms) / len(pending_ms)
    line["pending_ms"] = round(pend_avg, 3)
    line["pending"] = {"kernel": "k_pending<false> (ONCHIP tier, one wavefront per stream; every stream), "
                                 "k_pending<true> (HBM tier) for the streams rerun",
                       "ms_min": round(min(pending_ms), 3), "ms_max": round(max(pending_ms), 3),
                       "includes": "fx_pending_run (its launches, the status read back) and a synchronise "
                                   "(wall clock), after the executor step; not part of ms_per_step",
                       "nready": nready, "nopen": int(pend_h["nopen"].astype(np.uint64).sum()),
                       "errors": int(np.count_nonzero(pend_h["err"])),
                       "hbm_reruns": reruns, "hbm_rerun_share": round(reruns / S, 4),
                       "sample_peak_live_builders": peak_live,
                       "executed_rows_per_s": round(executed / (pend_avg * 1e-3), 1),
                       "alg_bytes_per_step": int(pend_bytes),
                       "alg_bytes_definition": "order, rifl and count words read and a head and a part word "
                                               "written per executed row (20 B), an index and a ready word per "
                                               "completed command, per stream nexec read and nready, nopen and "
                                               "err written",
                       "achieved_gbps": round(pend_bytes / (pend_avg * 1e-3) / 1e9, 3)}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "table_pending_bench.json"), "w") as out:
        json.dump({"what": "bench_table.py " + " ".join(sys.argv[1:]) + ": the line with the pending stage "
                           "(fx_pending_run after every executor step, over the step's own order plane, with the "
                           "rifl and the count of every row it names); pending_ms is wall time around the call and "
                           "a synchronise and is not part of ms_per_step",
                   "pending_ms": line["pending_ms"], "kv_ms": line.get("kv_ms"), "ms_per_step": line["ms_per_step"],
                   "nready": nready, "nopen": line["pending"]["nopen"],
                   "hbm_rerun_share": line["pending"]["hbm_rerun_share"], "line": line}, out, indent=1)
        out.write("\n")


def in_kernel(args, n, f, fq, thr, conflicts):
    """The `--shards G --in-kernel` line."""
    from fantoch_amd import _lib
    from fantoch_amd import device as fd
    from fantoch_amd import table as ft
    import table_resume
    import table_shapes_ps
    lib = _lib.load()
    G, D, per = args.shards, args.distinct, args.streams
    if 64 % G:
        raise SystemExit("--in-kernel: --shards must divide 64 (whole groups in every plane tile)")
    copies = per // D
    lag = args.msg_lag
    if args.device_synth:
        return in_kernel_run(args, n, f, fq, thr, conflicts, *device_groups(args, n, fq, conflicts))

    def delay(sender, dot, target, key):
        return (dot[0] * 7 + dot[1] * 13 + target * 5 + key * 3 + sender) % (lag + 1)

    t0 = time.time()
    groups = []
    for c in conflicts:
        for i in range(D // G):  # the seeds of `--shards G`
            sts, commands, _ = table_shapes_ps.synth_table_group(
                args.seed * 1000003 + 1000 * c + i, G, n, fq, thr, args.keys,
                table_shapes_ps.group_cmds(G, args.cmds), c, args.lag, args.window, args.kmax, G, args.msg_lag)
            groups.append((table_resume.own_events(sts), commands))
    small, route, targets, steps_out = ft.pack_table_groups(groups, n, args.keys, delay)
    gen_s = time.time() - t0
    steps, vmax, S = small.steps, small.vmax, per * len(conflicts)
    pw = _lib.plane_words(S, steps)
    tile_in = ((steps + 3) // 4) * 256
    tiles_small = small.S // 64
    src_tile = np.arange(tiles_small).repeat(copies)

    def upload(plane_small, nplanes=1):
        b = fd.DeviceBuffer(pw * nplanes * 4)
        for p in range(nplanes):
            big = plane_small[p * small.plane:(p + 1) * small.plane].reshape(tiles_small, tile_in)[src_tile]
            _lib.check(lib.fx_dev_h2d(b.ptr + p * pw * 4, np.ascontiguousarray(big).ctypes.data, pw * 4, None), "h2d")
        return b

    ins = [upload(small.hdr), upload(small.dot), upload(small.clock), upload(small.votes, 3 * vmax),
           upload(small.nkeys), upload(route)]
    lengths_h = small.lengths.reshape(tiles_small, 64)[src_tile].reshape(-1).astype(np.uint32)
    lengths, tg = fd.DeviceBuffer(S * 4), fd.DeviceBuffer(max(targets.nbytes, 4))
    lengths.upload(lengths_h)
    tg.upload(targets)

    def sample(s0):  # the group whose first stream is s0: own events, commands, delay rule; the input is as packed
        own, commands = groups[(int(src_tile[s0 // 64]) * 64 + s0 % 64) // G]
        return own, commands, delay, True

    config = {"distinct_groups": len(groups), "copies_of_each": copies, "generation_s": round(gen_s, 2)}
    return in_kernel_run(args, n, f, fq, thr, conflicts, ins + [tg, lengths], lengths_h, steps, vmax, steps_out,
                         len(targets), sample, config, None)


def device_groups(args, n, fq, conflicts):
    """The input of the `--device-synth --shards G --in-kernel` line, generated on the device."""
    from fantoch_amd import _lib
    from fantoch_amd import device as fd
    from fantoch_amd import table as ft
    import table_shapes_ps
    lib = _lib.load()
    G, per = args.shards, args.streams
    S = per * len(conflicts)
    # conflict_block = per / G: the groups of one conflict rate are adjacent
    synth = ft.table_group_synth_params(seed=args.seed, groups=S // G, shards=G, smax=G, n=n, fast_quorum=fq,
                                        keys=args.keys, cmds=table_shapes_ps.group_cmds(G, args.cmds), kmax=args.kmax,
                                        conflicts=conflicts, conflict_block=per // G, lag=args.lag, window=args.window,
                                        msg_lag=args.msg_lag)
    table = fd.DeviceTableGroups(synth)  # (the counting pass alone: the shapes of the buffers)
    gen_ms = []
    for _ in range(3):  # (the first is a warm-up)
        t1 = time.time()
        _lib.check(table.generate(), "fx_table_group_synth_generate")
        _lib.check(lib.fx_dev_synchronize(None), "sync")
        gen_ms.append(1e3 * (time.time() - t1))
    b = table.bufs
    ins = [b[name] for name in ("hdr", "dot", "clock", "votes", "nkeys", "route", "targets")] + [table.lengths]
    targets_h = b["targets"].download(np.uint32, table.targets_words)

    def sample(s0):
        """The group as the device holds it must be the generator's restatement as pack_table_groups packs it."""
        own, commands, delays = ft.synth_table_groups_c6(synth, s0 // G)
        planes, route = table.download_tile(s0 // 64)
        want, want_route, want_targets, _ = ft.pack_table_groups([(own, commands)], n, args.keys, delays)
        ok = True
        for h in range(G):
            s = s0 % 64 + h
            ok = ok and planes.stream(s) == own[h] == want.stream(h)
            for r in range(len(own[h])):
                i, j = int(route[_lib.index(r, s, planes.steps)]), int(want_route[_lib.index(r, h, want.steps)])
                if j == _lib.FX_TABLE_ROUTE_NONE or i == _lib.FX_TABLE_ROUTE_NONE:
                    ok = ok and i == j
                else:
                    m = int(want_targets[j])
                    ok = ok and i + 1 + m <= len(targets_h) and \
                        np.array_equal(targets_h[i:i + 1 + m], want_targets[j:j + 1 + m])
        return own, commands, delays, ok

    config = {"distinct_groups": S // G, "copies_of_each": 1, "generation_s": None}
    generation = {"kernel": "k_table_group_synth (counting pass, emitting pass), one lane per group",
                  "ms_runs": [round(x, 3) for x in gen_ms],
                  "includes": "both passes, the prefix over the groups on the host, the fill of the planes and the "
                              "counts read back",
                  "targets_words": int(table.targets_words)}
    return (ins, table.lengths.download(np.uint32, S), table.steps, table.vmax, table.steps_out, table.targets_words,
            sample, config, generation)


def in_kernel_run(args, n, f, fq, thr, conflicts, ins, lengths_h, steps, vmax, steps_out, targets_words, sample,
                  config, generation):
    """One fx_table_run_groups per step over device buffers (hdr, dot, clock, votes, nkeys, route, targets,
    lengths), the sample against closed_loop, and the line."""
    from fantoch_amd import _lib
    from fantoch_amd import device as fd
    from fantoch_amd import table as ft
    import table_resume
    lib = _lib.load()
    G, per, lag = args.shards, args.streams, args.msg_lag
    S = per * len(conflicts)
    ow = _lib.plane_words(S, steps_out)
    tile_out = ((steps_out + 3) // 4) * 256
    tg, lengths = ins[6], ins[7]
    planes = {name: fd.DeviceBuffer(ow * 4) for name in ("order", "release", "stable_sent", "handled_src", "handled_dot")}
    per_stream = {name: fd.DeviceBuffer(S * 4) for name in ("nexec", "err", "handled_len")}
    stable, rounds = fd.DeviceBuffer(S * args.keys * 4), fd.DeviceBuffer(S // G * 4)
    state = fd.DeviceBuffer(lib.fx_table_groups_state_bytes(n, args.keys, S))
    inb = _lib.TableGroupBatch(
        _lib.TableBatchMk(_lib.TableBatch(ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, lengths.ptr, S, steps, n,
                                          args.keys, vmax, thr), ins[4].ptr),
        ins[5].ptr, tg.ptr, targets_words, G, steps_out)
    outb = _lib.TableGroupOut(_lib.OrderBatch(planes["order"].ptr, planes["release"].ptr, per_stream["nexec"].ptr,
                                              per_stream["err"].ptr), stable.ptr, planes["stable_sent"].ptr,
                              planes["handled_src"].ptr, planes["handled_dot"].ptr, per_stream["handled_len"].ptr,
                              rounds.ptr)

    def step():
        _lib.check(lib.fx_table_run_groups(ctypes.byref(inb), ctypes.byref(outb), state.ptr, 0, None),
                   "fx_table_run_groups")
        _lib.check(lib.fx_dev_synchronize(None), "sync")

    for _ in range(max(args.warmup, 1)):
        step()
    pending_ms = []
    if args.pending:
        # A group's order names handled rows.  Every step handles the same input the same way, so the rifl and
        # the count of every handled row are gathered once, here: an own row's from the dot and nkeys planes
        # through handled_src, a routed message's rifl from handled_dot with count 0 (nobody waits for it).
        tile_in, s4 = ((steps + 3) // 4) * 256, (steps_out + 3) // 4
        hlen = per_stream["handled_len"].download(np.uint32, S)
        rifl_d, count_d = fd.DeviceBuffer(ow * 4), fd.DeviceBuffer(ow * 4)
        w = np.arange(tile_out, dtype=np.int64)
        lane, row = (w >> 2) & 63, (w >> 8) * 4 + (w & 3)  # (w >> 8 < s4: one tile of 64 streams)
        assert tile_out == s4 * 256

        def tile(buf, t, words):
            out = np.empty(words, np.uint32)
            _lib.check(lib.fx_dev_d2h(out.ctypes.data, buf.ptr + t * words * 4, words * 4, None), "d2h")
            _lib.check(lib.fx_dev_synchronize(None), "sync")
            return out

        for t in range(S // 64):
            src, hdot = tile(planes["handled_src"], t, tile_out), tile(planes["handled_dot"], t, tile_out)
            dot_in, nkeys_in = tile(ins[1], t, tile_in), tile(ins[4], t, tile_in)
            valid = row < hlen[t * 64 + lane]
            own = valid & ((src & _lib.FX_TABLE_HANDLED_MSG) == 0)
            at = _lib.index(np.where(own, np.minimum(src, steps - 1), 0), lane, steps)
            rifl_t = np.where(own, dot_in[at], np.where(valid, hdot, 0)).astype(np.uint32)
            count_t = np.where(own, nkeys_in[at], 0).astype(np.uint32)
            for buf, arr in ((rifl_d, rifl_t), (count_d, count_t)):
                _lib.check(lib.fx_dev_h2d(buf.ptr + t * tile_out * 4, arr.ctypes.data, tile_out * 4, None), "h2d")
            _lib.check(lib.fx_dev_synchronize(None), "sync")
        pend_out, pending_step, pend_reruns = pending_setup(fd, _lib, planes["order"], per_stream["nexec"], rifl_d,
                                                            count_d, 0xFF, S, steps_out)
        pending_step()
    lib.fx_profile_enable(1)
    kms = []
    t0 = time.time()
    for _ in range(args.steps):
        step()
        if args.pending:
            pending_ms.append(pending_step())
        ms = ctypes.c_float()
        if lib.fx_profile_slot_ms(_lib.FX_PROFILE_SLOT_TABLE + 3, ctypes.byref(ms)) == 0:
            kms.append(ms.value)
    step_s = (time.time() - t0 - 1e-3 * sum(pending_ms)) / args.steps  # (the stage is reported beside the step)
    lib.fx_profile_enable(0)

    got = {name: b.download(np.uint32, S) for name, b in per_stream.items()}
    stable_h = stable.download(np.uint32, S * args.keys).reshape(S, args.keys)
    rounds_h = rounds.download(np.uint32, S // G)
    handled, executed = int(got["handled_len"].sum()), int(got["nexec"].sum())

    def tile_of(buf, t):
        out = np.empty(tile_out, np.uint32)
        _lib.check(lib.fx_dev_d2h(out.ctypes.data, buf.ptr + t * tile_out * 4, tile_out * 4, None), "d2h")
        _lib.check(lib.fx_dev_synchronize(None), "sync")
        return out

    if args.pending:
        import pending_ref
        from fantoch_amd import pending as fp
        pend_h = {name: pend_out[name].download(np.uint32, S) for name in ("nready", "nopen", "err")}
        peak_live = 0
    def rows_all(s):
        return _lib.index(np.arange(steps_out), s % 64, steps_out)

    # parity sample: `--sample` groups per conflict rate, spread over the copies
    parity, checked, attached = True, 0, 0
    for ci in range(len(conflicts)):
        for j in range(args.sample):
            s0 = (ci * per + (j * 977 + 13 * ci) % per) // G * G  # the group's first stream
            own, commands, delay, input_ok = sample(s0)
            parity = parity and input_ok
            want_streams, want = table_resume.closed_loop(own, commands, n, thr, args.keys, delay)
            tiles = {name: tile_of(b, s0 // 64) for name, b in planes.items()}
            for h in range(G):
                s, ref = s0 + h, want[h]
                L, ne = int(got["handled_len"][s]), int(got["nexec"][s])
                rows = _lib.index(np.arange(L), s % 64, steps_out)
                stream = ft.handled_stream(own[h], tiles["handled_src"][rows], tiles["handled_dot"][rows])
                none = _lib.FX_RELEASE_NONE
                ok = (stream == want_streams[h] and int(got["err"][s]) == ref["err"] and ne == ref["nexec"]
                      and [int(x) & ~_lib.FX_ORDER_SCC_START for x in tiles["order"][rows[:ne]]] == ref["order"]
                      and {a: int(v) for a, v in enumerate(tiles["release"][rows]) if v != none} == ref["release"]
                      and {a: int(v) for a, v in enumerate(tiles["stable_sent"][rows]) if v != none} == ref["sent"]
                      and stable_h[s].tolist() == ref["stable"])
                if args.pending and ref["err"] == 0:  # heads, parts and the ready list against the restatement
                    evs = want_streams[h]
                    pw_ref = pending_ref.run(ref["order"], [_lib.pack_dot(*e[2]) if e[0] != "D" else 0 for e in evs],
                                             [(e[5] if len(e) > 5 else 1) if e[0] == "A" else 0 for e in evs],
                                             steps_out)
                    peak_live = max(peak_live, pw_ref["peak"])
                    head_rows, ready_rows = (tile_of(pend_out[name], s0 // 64)[rows_all(s)]
                                             for name in ("head", "ready"))
                    part_rows = [tile_of(pend_out["part"], j * (ow // tile_out) + s0 // 64)[rows_all(s)]
                                 for j in range(fp.MAX_PARTS)]
                    ok = ok and pending_sample_ok(pw_ref, pend_h, s, head_rows, ready_rows, part_rows)
                parity, checked = parity and ok, checked + 1
                attached += sum(ev[0] == "A" for ev in own[h]) - ne
    k_main = sum(kms) / len(kms) if kms else None
    line = {
        "metric": "events/sec, Tempo TableExecutor, closed-loop shard groups in one launch (fx_table_run_groups)",
        "value": round(handled / step_s, 1), "unit": "events/s", "higher_is_better": True,
        "executed_cmds_per_s": round(executed / step_s, 1), "ms_per_step": round(step_s * 1e3, 3),
        "steps": args.steps, "warmup": args.warmup, "n_gpus": 1, "dtype": "u32",
        "errors": int(np.count_nonzero(got["err"])),
        "error_codes": {str(int(c)): int(np.count_nonzero(got["err"] == c)) for c in np.unique(got["err"]) if c},
        "max_rounds": int(rounds_h.max()), "own_events_per_step": int(lengths_h.sum()),
        "events_per_step": handled, "executed_per_step": executed,
        "config": {"workload": "TableExecutor, n=%d f=%d (fast quorum %d, stability threshold %d), %d streams x "
                               "conflict %s %%, groups of %d shard executors, %d cmds/executor of 1..%d keys per shard, "
                               "%d keys, lag %d, window %d, messages 0..%d rounds late"
                               % (n, f, fq, thr, per, conflicts, G, args.cmds, args.kmax, args.keys, args.lag,
                                  args.window, lag),
                   "shards_per_group": G, "msg_lag": lag, "streams": S, "groups": S // G,
                   "own_events_per_stream": steps, "rows_per_output_plane": steps_out, "vmax": vmax,
                   "distinct_groups": config["distinct_groups"], "copies_of_each": config["copies_of_each"],
                   "generation_s": config["generation_s"],
                   "parallelism": "one workgroup per group, one wavefront per shard executor"},
        "kernel": {"name": "k_table_group (after k_table_group_check)", "kernel_ms_avg": round(k_main, 3) if k_main else None,
                   "kernel_ms_min": round(min(kms), 3) if kms else None,
                   "kernel_ms_max": round(max(kms), 3) if kms else None},
        "sample_parity": bool(parity), "sample_streams": checked,
    }
    if args.pending:
        pending_report(line, pending_ms, pend_h, int(pend_reruns.value), S, executed, peak_live)
    if generation:
        line["generation_ms"] = round(min(generation["ms_runs"][1:]), 3)
        line["generation"] = generation
        stops = int(np.count_nonzero(got["err"] == _lib.FX_ERR_CAPACITY))
        line["capacity_stops"], line["capacity_stop_share"] = stops, round(stops / S, 6)
        line["sample_attached_not_executed"] = attached  # attached events of the sampled streams left unexecuted
    print(json.dumps(line), flush=True)
    return 0 if parity else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=4096, help="streams per conflict rate")
    ap.add_argument("--distinct", type=int, default=64, help="generated streams per conflict rate")
    ap.add_argument("--conflicts", default="0,2,10,50,100")
    ap.add_argument("--cmds", type=int, default=1000)
    ap.add_argument("--keys", type=int, default=16)
    ap.add_argument("--lag", type=int, default=6)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--kmax", type=int, default=1, help="keys per command 1..kmax; above 1: fx_table_run_mk")
    ap.add_argument("--shards", type=int, default=1, help="shard executors per group; above 1: fx_table_run_ps")
    ap.add_argument("--msg-lag", type=int, default=3, help="--shards: rounds a StableAtShard message may be late")
    ap.add_argument("--in-kernel", action="store_true",
                    help="with --shards: the closed loop of every group in one fx_table_run_groups launch")
    ap.add_argument("--chunks", type=int, default=0, help="above 0: the HBM tier in this many fx_table_advance calls")
    ap.add_argument("--device-synth", action="store_true",
                    help="generate every stream on the device (fx_table_synth_generate), all distinct")
    ap.add_argument("--kv", action="store_true", help="run the KV stage (fx_kv_execute) after each executor step")
    ap.add_argument("--read-pct", type=int, default=50, help="--kv: percent of GETs")
    ap.add_argument("--delete-pct", type=int, default=10, help="--kv: percent of DELETEs")
    ap.add_argument("--pending", action="store_true",
                    help="run the pending stage (fx_pending_run) after each executor step; needs --kmax above 1")
    ap.add_argument("--sample", type=int, default=5, help="streams per conflict rate checked against the restatement")
    args = ap.parse_args()

    from fantoch_amd import _lib
    from fantoch_amd import device as fd
    from fantoch_amd import table as ft
    import table_ref
    import table_ref_mk

    ps = args.shards > 1
    if args.device_synth and ps and not args.in_kernel:
        raise SystemExit("--device-synth with --shards needs --in-kernel: the host-paced streams of a group hold the "
                         "StableAtShard messages, which depend on the executors' own stable_sent; only a group's own "
                         "events (the input of --in-kernel) are generated")
    multi = args.kmax > 1 or ps
    if args.kv and (ps or args.chunks):
        raise SystemExit("--kv goes with the single-key and --kmax lines (no --shards, no --chunks)")
    if args.pending and (args.kmax < 2 or args.chunks):
        raise SystemExit("--pending goes with --kmax above 1 and without --chunks")
    lib = _lib.load()
    if lib.fx_device_count() <= 0:
        raise SystemExit("no GPU visible to libfantoch_amd")
    n, f = 5, 1
    fq, _, thr = ft.tempo_quorum_sizes(n, f)
    conflicts = [int(c) for c in args.conflicts.split(",")]
    D, per = args.distinct, args.streams
    if args.device_synth:
        D = per  # every stream is generated, none is copied
    if D % 64 or per % D:
        raise SystemExit("--distinct must be a multiple of 64 and divide --streams")
    copies = per // D
    if args.in_kernel:
        if not ps or args.chunks:
            raise SystemExit("--in-kernel goes with --shards G (G > 1) and without --chunks")
        return in_kernel(args, n, f, fq, thr, conflicts)
    t0 = time.time()
    table = None
    if args.device_synth:
        # conflict_block = per: the streams of one conflict rate are adjacent, as below
        synth = ft.table_synth_params(seed=args.seed, streams=per * len(conflicts), n=n, fast_quorum=fq,
                                      keys=args.keys, cmds=args.cmds, kmax=args.kmax, conflicts=conflicts,
                                      conflict_block=per, lag=args.lag, window=args.window)
        table = fd.DeviceTable(synth)  # (the counting pass alone: the longest stream is the planes' steps)
        gen_ms = []
        for _ in range(3):  # (the first is a warm-up)
            t1 = time.time()
            _lib.check(table.generate(), "fx_table_synth_generate")
            _lib.check(lib.fx_dev_synchronize(None), "sync")
            gen_ms.append(1e3 * (time.time() - t1))
        streams, small = None, None
    elif ps:
        import table_ref_ps
        import table_shapes_ps
        G = args.shards
        streams = []
        for c in conflicts:
            mine = []
            for i in range((D + G - 1) // G):  # whole groups; the last one may lose streams to the tile size
                mine += table_shapes_ps.synth_table_group(
                    args.seed * 1000003 + 1000 * c + i, G, n, fq, thr, args.keys,
                    table_shapes_ps.group_cmds(G, args.cmds), c, args.lag, args.window, args.kmax, G, args.msg_lag)[0]
            streams += mine[:D]
    elif multi:
        streams = [ft.synth_table_streams_mk(args.seed * 1000003 + 1000 * c + i, n, fq, args.keys, args.cmds, c,
                                             args.lag, args.window, args.kmax) for c in conflicts for i in range(D)]
    else:
        streams = [ft.synth_table_streams(args.seed * 1000003 + 1000 * c + i, n, fq, args.keys, args.cmds, c, args.lag,
                                          args.window) for c in conflicts for i in range(D)]
    if table is None:
        small = ft.pack_table_streams(streams, n, args.keys)
    gen_s = time.time() - t0
    steps, vmax = (table.steps, table.vmax) if table else (small.steps, small.vmax)
    S = per * len(conflicts)
    pw = _lib.plane_words(S, steps)
    tile_words = ((steps + 3) // 4) * 256
    tiles_small = S // 64 if table else small.S // 64
    # tile t of the launch = tile (t // copies) of the generated batch: a conflict rate's streams stay adjacent
    src_tile = np.arange(tiles_small).repeat(copies)

    def upload(plane_small, nplanes=1):
        b = fd.DeviceBuffer(pw * nplanes * 4)
        for p in range(nplanes):
            big = plane_small[p * small.plane:(p + 1) * small.plane].reshape(tiles_small, tile_words)[src_tile]
            _lib.check(lib.fx_dev_h2d(b.ptr + p * pw * 4, np.ascontiguousarray(big).ctypes.data, pw * 4, None), "h2d")
        return b

    if table:
        hdr, dot, clock, votes = (table.bufs[name] for name in ("hdr", "dot", "clock", "votes"))
        lengths = table.lengths
        lengths_h = lengths.download(np.uint32, S)
    else:
        hdr, dot, clock = upload(small.hdr), upload(small.dot), upload(small.clock)
        votes = upload(small.votes, 3 * vmax)
        lengths_h = small.lengths.reshape(tiles_small, 64)[src_tile].reshape(-1).astype(np.uint32)
        lengths = fd.DeviceBuffer(S * 4)
        lengths.upload(lengths_h)
    order, release = fd.DeviceBuffer(pw * 4), fd.DeviceBuffer(pw * 4)
    nexec, err, stable = fd.DeviceBuffer(S * 4), fd.DeviceBuffer(S * 4), fd.DeviceBuffer(S * args.keys * 4)
    order.zero()
    release.fill_bytes(0xFF)
    inb = _lib.TableBatch(hdr.ptr, dot.ptr, clock.ptr, votes.ptr, lengths.ptr, S, steps, n, args.keys, vmax, thr)
    run_fn = lib.fx_table_run
    if multi:
        nkeys = table.nkeys if table else upload(
            small.nkeys if small.nkeys is not None else
            np.full(small.plane, ft.table_ps_word(1, 1) if ps else 1, np.uint32))
        inb = _lib.TableBatchMk(inb, nkeys.ptr)
        run_fn = lib.fx_table_run_mk
    if ps:
        sent = fd.DeviceBuffer(pw * 4)
        sent.fill_bytes(0xFF)
        run_fn = lambda i, o, st, *rest: lib.fx_table_run_ps(i, o, st, sent.ptr, *rest)
    outb = _lib.OrderBatch(order.ptr, release.ptr, nexec.ptr, err.ptr)
    reruns = ctypes.c_uint32()

    def step():
        _lib.check(run_fn(ctypes.byref(inb), ctypes.byref(outb), stable.ptr, 0, None, ctypes.byref(reruns)),
                   "fx_table_run")

    kv_ms = []
    if args.kv:
        kv_ops = fd.synth_kv_ops(args.seed, S, steps, args.read_pct, args.delete_pct, lengths=lengths)
        kv_out = {"result": fd.DeviceBuffer(pw * 4), "store": fd.DeviceBuffer(S * args.keys * 4),
                  "monitor": fd.DeviceBuffer(pw * 4), "mon_off": fd.DeviceBuffer(S * (args.keys + 1) * 4),
                  "err": fd.DeviceBuffer(S * 4)}
        kv_in = _lib.KvBatch(order.ptr, nexec.ptr, hdr.ptr, 0x00FFFFFF, kv_ops.ptr, S, steps, args.keys, 1)
        kv_outb = _lib.KvOut(*(kv_out[name].ptr for name in ("result", "store", "monitor", "mon_off", "err")))

        def kv_step():
            t1 = time.time()
            _lib.check(lib.fx_kv_execute(ctypes.byref(kv_in), ctypes.byref(kv_outb), None), "fx_kv_execute")
            _lib.check(lib.fx_dev_synchronize(None), "sync")
            return 1e3 * (time.time() - t1)

    pending_ms = []
    if args.pending:
        from fantoch_amd import pending as fp
        pend_mask = 0xFF if ps else 0xFFFFFFFF
        pend_out, pending_step, pend_reruns = pending_setup(fd, _lib, order, nexec, dot, nkeys, pend_mask, S, steps)

    whole_ms = None
    if args.chunks:
        C = args.chunks
        kind = _lib.FX_TABLE_KIND_PS if ps else _lib.FX_TABLE_KIND_MK if multi else _lib.FX_TABLE_KIND_SINGLE
        # the streams whole at the HBM tier, for comparison
        wstate = fd.DeviceBuffer((lib.fx_table_state_bytes_ps if ps else lib.fx_table_state_bytes)(n, args.keys, S))
        wargs = (ctypes.byref(inb), ctypes.byref(outb), stable.ptr) + ((sent.ptr,) if ps else ()) + \
            (None, S, _lib.FX_TABLE_TIER_HBM, wstate.ptr, 0, None)
        wfn = lib.fx_table_execute_ps if ps else lib.fx_table_execute_mk if multi else lib.fx_table_execute
        times = []
        for _ in range(1 + args.steps):  # (the first is a warm-up)
            t1 = time.time()
            _lib.check(wfn(*wargs), "fx_table_execute")
            _lib.check(lib.fx_dev_synchronize(None), "sync")
            times.append(time.time() - t1)
        whole_ms = 1e3 * sum(times[1:]) / args.steps
        wstate.free()
        state_bytes = lib.fx_table_session_bytes(kind, n, args.keys, S)
        state = fd.DeviceBuffer(state_bytes)
        pieces = []
        for i in range(C):
            cut = fd.DeviceBuffer(S * 4)
            cut.upload(((lengths_h.astype(np.uint64) * (i + 1) + C - 1) // C).astype(np.uint32))
            b = _lib.TableBatch(hdr.ptr, dot.ptr, clock.ptr, votes.ptr, cut.ptr, S, steps, n, args.keys, vmax, thr)
            pieces.append((cut, _lib.TableBatchMk(b, nkeys.ptr if multi else None)))

        def step():  # noqa: F811
            for i, (_, b) in enumerate(pieces):
                _lib.check(lib.fx_table_advance(ctypes.byref(b), kind, ctypes.byref(outb), stable.ptr,
                                                sent.ptr if ps else None, state.ptr,
                                                _lib.FX_FLAG_INIT if i == 0 else 0, None), "fx_table_advance")
            _lib.check(lib.fx_dev_synchronize(None), "sync")

    for _ in range(max(args.warmup, 1)):
        step()
        if args.kv:
            kv_step()
        if args.pending:
            pending_step()
    lib.fx_profile_enable(1)
    kms, hms = [], []
    t0 = time.time()
    for _ in range(args.steps):
        step()
        if args.kv:
            _lib.check(lib.fx_dev_synchronize(None), "sync")
            kv_ms.append(kv_step())
        if args.pending:
            _lib.check(lib.fx_dev_synchronize(None), "sync")
            pending_ms.append(pending_step())
        ms = ctypes.c_float()
        if lib.fx_profile_slot_ms(_lib.FX_PROFILE_SLOT_TABLE + _lib.FX_TABLE_TIER_ONCHIP, ctypes.byref(ms)) == 0:
            kms.append(ms.value)
        if reruns.value and lib.fx_profile_slot_ms(_lib.FX_PROFILE_SLOT_TABLE + _lib.FX_TABLE_TIER_HBM,
                                                   ctypes.byref(ms)) == 0:
            hms.append(ms.value)
    # (the KV and pending stages are reported beside the step, not in it)
    elapsed = time.time() - t0 - 1e-3 * (sum(kv_ms) + sum(pending_ms))
    lib.fx_profile_enable(0)

    nexec_h, err_h = nexec.download(np.uint32, S), err.download(np.uint32, S)
    events, executed = int(lengths_h.sum()), int(nexec_h.sum())

    # parity sample: `--sample` streams per conflict rate, spread over the copies
    def tile_of(buf, t):
        out = np.empty(tile_words, np.uint32)
        _lib.check(lib.fx_dev_d2h(out.ctypes.data, buf.ptr + t * tile_words * 4, tile_words * 4, None), "d2h")
        _lib.check(lib.fx_dev_synchronize(None), "sync")
        return out

    stable_h = stable.download(np.uint32, S * args.keys).reshape(S, args.keys)
    parity, checked = True, 0
    if args.kv:
        import kv_ref
        from fantoch_amd import kv as fk
        kv_h = fk.KvResult(S, steps, args.keys, 1, None, kv_out["store"].download(np.uint32, S * args.keys), None,
                           kv_out["mon_off"].download(np.uint32, S * (args.keys + 1)),
                           kv_out["err"].download(np.uint32, S), 0)
        kv_writes = int(kv_h.mon_off[:, args.keys].astype(np.uint64).sum()) if not np.count_nonzero(kv_h.err) else 0
    if args.pending:
        import pending_ref
        pend_h = {name: pend_out[name].download(np.uint32, S) for name in ("nready", "nopen", "err")}
        peak_live = 0
    for ci in range(len(conflicts)):
        for j in range(args.sample):
            s = ci * per + (j * 977 + 13 * ci) % per
            src = int(src_tile[s // 64]) * 64 + s % 64
            if table:  # the stream as the device holds it, which must be the generator's restatement
                stream = table.download_tile(s // 64).stream(s % 64)
                parity = parity and stream == ft.synth_table_streams_c6(synth, s)
            else:
                stream = streams[src]
            ref = (table_ref_ps if ps else table_ref_mk if multi else table_ref).run_stream(stream, n, thr, args.keys)
            o, r = tile_of(order, s // 64), tile_of(release, s // 64)
            rows = _lib.index(np.arange(steps), s % 64, steps)
            want_o = np.array(ref["order"], np.uint32) | np.uint32(_lib.FX_ORDER_SCC_START)
            want_r = np.full(steps, _lib.FX_RELEASE_NONE, np.uint32)
            for a, st in ref["release"].items():
                want_r[a] = st
            ok = (int(err_h[s]) == ref["err"] and int(nexec_h[s]) == ref["nexec"]
                  and np.array_equal(o[rows][:ref["nexec"]], want_o) and np.array_equal(r[rows], want_r)
                  and stable_h[s].tolist() == ref["stable"])
            if ps:
                want_s = np.full(steps, _lib.FX_RELEASE_NONE, np.uint32)
                for a, st in ref["sent"].items():
                    want_s[a] = st
                ok = ok and np.array_equal(tile_of(sent, s // 64)[rows], want_s)
            if args.kv:  # results, store and monitors of the stream against the restatement over the device's order
                exec_order = [int(x) & 0x7FFFFFFF for x in o[rows][:int(nexec_h[s])]]
                op_rows = tile_of(kv_ops, s // 64)[rows]
                ops_of = [[int(w)] if fk.op_kind(w) != fk.EMPTY else [] for w in op_rows]
                want_res, want_store, want_mon = kv_ref.run(exec_order, [ev[1] for ev in stream], ops_of[:len(stream)])
                res_rows, mon_rows = tile_of(kv_out["result"], s // 64)[rows], tile_of(kv_out["monitor"], s // 64)[rows]
                off = kv_h.mon_off[s]
                ok = (ok and int(kv_h.err[s]) == 0 and all(int(res_rows[a]) == want_res[a][0] for a in exec_order)
                      and kv_h.store[s].tolist() == [want_store.get(k, 0) for k in range(args.keys)]
                      and int(off[0]) == 0
                      and all(mon_rows[int(off[k]):int(off[k + 1])].tolist() == want_mon.get(k, [])
                              for k in range(args.keys)))
            if args.pending:  # heads, parts and the ready list against the restatement over the device's order
                exec_order = [int(x) & 0x7FFFFFFF for x in o[rows][:int(nexec_h[s])]]
                want = pending_ref.run(exec_order, [int(x) for x in tile_of(dot, s // 64)[rows]],
                                       [int(x) & pend_mask for x in tile_of(nkeys, s // 64)[rows]], steps)
                peak_live = max(peak_live, want["peak"])
                head_rows, ready_rows = (tile_of(pend_out[name], s // 64)[rows] for name in ("head", "ready"))
                part_rows = [tile_of(pend_out["part"], j * (pw // tile_words) + s // 64)[rows]
                             for j in range(fp.MAX_PARTS)]
                ok = ok and pending_sample_ok(want, pend_h, s, head_rows, ready_rows, part_rows)
            parity, checked = parity and ok, checked + 1

    k_main = sum(kms) / len(kms) if kms else None
    step_s = elapsed / args.steps
    # input planes read once (hdr, dot, clock, 3 * vmax vote planes: 4 bytes per
    # event each), outputs written once (order + release per executed command,
    # nexec + err + the stable clocks per stream)
    alg_bytes = 4.0 * (3 + 3 * vmax + (1 if multi else 0)) * events + 8.0 * executed + (8.0 + 4.0 * args.keys) * S
    if ps:
        alg_bytes += 4.0 * sum(ev[0] == "A" for st in streams for ev in st) * copies  # stable_sent, at most
    achieved = alg_bytes / ((k_main * 1e-3) if k_main else step_s) / 1e9
    line = {
        "metric": "events/sec, Tempo TableExecutor over batched streams (%s)" % (
            "fx_table_run_ps" if ps else "fx_table_run_mk" if multi else "fx_table_run"),
        "value": round(events / step_s, 1), "unit": "events/s", "higher_is_better": True,
        "executed_cmds_per_s": round(executed / step_s, 1), "ms_per_step": round(step_s * 1e3, 3),
        "steps": args.steps, "warmup": args.warmup, "n_gpus": 1, "dtype": "u32",
        "reruns": int(reruns.value), "errors": int(np.count_nonzero(err_h)),
        "events_per_step": events, "executed_per_step": executed,
        "config": {"workload": "TableExecutor, n=%d f=%d (fast quorum %d, stability threshold %d), %d streams x "
                               "conflict %s %%, %d cmds/stream of 1..%d keys, %d keys, lag %d, window %d"
                               % (n, f, fq, thr, per, conflicts, args.cmds, args.kmax, args.keys, args.lag,
                                  args.window),
                   "shards_per_group": args.shards, "msg_lag": args.msg_lag if ps else None,
                   "streams": S, "events_per_stream": steps, "vmax": vmax,
                   "distinct_streams": S if table else len(streams), "copies_of_each": copies,
                   "generation_s": round(gen_s, 2),
                   "parallelism": "one wavefront per stream, 4 streams per workgroup"},
        "roofline": {"bound": "hbm", "achieved": round(achieved, 3), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBPS, 6), "kernel": "k_table<false, 1, 4, %s> (ONCHIP tier; every stream)" % (
                         "true, true" if ps else "true" if multi else "false"),
                     "kernel_ms_avg": round(k_main, 3) if k_main else None,
                     "kernel_ms_min": round(min(kms), 3) if kms else None,
                     "kernel_ms_max": round(max(kms), 3) if kms else None,
                     "hbm_rerun_ms_avg": round(sum(hms) / len(hms), 3) if hms else None,
                     "alg_bytes_per_step": int(alg_bytes),
                     "alg_bytes_definition": "input planes read once (4 B x (3 + 3 vmax) per event), order + release "
                                             "written once per executed command, nexec + err + stable clocks per stream"},
        "sample_parity": bool(parity), "sample_streams": checked,
    }
    if table:
        line["generation_ms"] = round(min(gen_ms[1:]), 3)
        line["generation"] = {"kernel": "k_table_synth (counting pass, emitting pass), one lane per stream",
                              "ms_runs": [round(x, 3) for x in gen_ms],
                              "includes": "both passes, the zero fill of the planes and the lengths read back",
                              "rerun_share": round(int(reruns.value) / S, 4)}
    if args.kv:
        # order, key and op word read and one result word written per executed row, one monitor word per write
        # partial; per stream nexec read, err, the final store and the monitor offsets written
        kv_bytes = 16.0 * executed + 4.0 * kv_writes + (8.0 + 4.0 * (2 * args.keys + 1)) * S
        kv_avg = sum(kv_ms) / len(kv_ms)
        line["kv_ms"] = round(kv_avg, 3)
        line["kv"] = {"kernel": "k_kv_exec<%s> (one wavefront per stream)" % (
                          "LDS" if args.keys <= _lib.FX_KV_ONCHIP_KEYS else "HBM"),
                      "ms_min": round(min(kv_ms), 3), "ms_max": round(max(kv_ms), 3),
                      "includes": "the launch and a synchronise around it (wall clock), after the executor step; "
                                  "not part of ms_per_step",
                      "read_pct": args.read_pct, "delete_pct": args.delete_pct, "omax": 1,
                      "executed_rows_per_s": round(executed / (kv_avg * 1e-3), 1),
                      "write_partials_per_step": kv_writes, "errors": int(np.count_nonzero(kv_h.err)),
                      "alg_bytes_per_step": int(kv_bytes),
                      "alg_bytes_definition": "order, key and op words read and a result word written per executed "
                                              "row (16 B), a monitor word per write partial, per stream nexec read and "
                                              "err, store[keys] and mon_off[keys + 1] written",
                      "achieved_gbps": round(kv_bytes / (kv_avg * 1e-3) / 1e9, 3)}
    if args.pending:
        pending_report(line, pending_ms, pend_h, int(pend_reruns.value), S, executed, peak_live)
    if args.chunks:
        line["metric"] = "events/sec, Tempo TableExecutor, HBM tier in %d fx_table_advance calls per stream" % args.chunks
        line["roofline"]["kernel"] = "k_table<true, 8, 1, ..., RESUME> (HBM tier; every stream, %d calls)" % args.chunks
        line["chunks"] = {"calls_per_step": args.chunks, "ms_per_step": round(step_s * 1e3, 3),
                          "whole_hbm_ms_per_step": round(whole_ms, 3), "state_bytes_per_call": int(state_bytes),
                          "state_traffic_bytes_per_step": int(2 * state_bytes * args.chunks),
                          "status": "ok" if not np.count_nonzero(err_h) else "stream errors"}
    print(json.dumps(line), flush=True)
    return 0 if parity else 1


if __name__ == "__main__":
    sys.exit(main())
