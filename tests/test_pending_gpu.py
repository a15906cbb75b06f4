"""The pending stage on the device (fx_pending_aggregate, fx_pending_run): every
output byte against the host twin, and both against the restatement of
aggregate.rs (pending_ref); behind the table executor, a closed-loop shard
group and a device-generated batch end to end.  Every buffer, the HBM tier's
state included, starts as 0xA5 bytes and the register file is filled with
garbage before the launches.  GPU only."""
import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import kv as K
from fantoch_amd import pending as P
from fantoch_amd import table as ft

import kv_shapes as KS
import pending_ref
import pending_shapes as PS
import table_resume as TR
import table_shapes as T
import table_shapes_ps as TP
from test_sim_poison import FILLS, poisoner

pytestmark = pytest.mark.gpu

CASES = PS.all_cases()
RUNS = [(i, t) for i, c in enumerate(CASES) for t in c.tiers]
TIER_NAME = {PS.ONCHIP: "onchip", PS.HBM: "hbm", None: "run"}


def same_bytes(dev, host):
    for name in P.NAMES:
        a, b = getattr(dev, name), getattr(host, name)
        assert np.array_equal(a, b), "%s differs at word %d" % (name, int(np.flatnonzero(a != b)[0]))


def run_case(case, tier, fill=FILLS[0], **kw):
    return fd.run_pending(case.order, case.nexec, case.rifl, case.count, case.S, case.steps, case.count_mask,
                          case.process, fill=0xA5, before_launch=poisoner(*fill), tier=tier, **kw)


@pytest.mark.parametrize("i,tier", RUNS, ids=["%s %s" % (CASES[i].name, TIER_NAME[t]) for i, t in RUNS])
def test_device_equals_host_twin_and_restatement(gpu, i, tier):
    case = CASES[i]
    dev = run_case(case, tier, FILLS[(i + (tier or 2)) % len(FILLS)])
    same_bytes(dev, case.run_host(tier))
    case.check(dev, tier)
    if tier is None:  # the streams that ran out of builders, and no others, ran again
        assert dev.reruns == sum(case.restated(s, PS.ONCHIP)["err"] == PS.C for s in range(case.S))


def test_every_fill_of_the_register_file(gpu):
    case = PS.reuse()
    for tier in case.tiers:
        host = case.run_host(tier)
        case.check(host, tier)
        for fill in FILLS:
            same_bytes(run_case(case, tier, fill), host)


def test_stream_map_covers_a_subset(gpu):
    """HBM tier: lane l of the launch runs stream stream_map[l] on the l-th table; the other streams keep 0xA5."""
    for case, chosen in ((PS.hbm_buckets(), [2, 0]), (PS.chunk_edges(65), [64, 3, 5, 10, 11])):
        dev = run_case(case, PS.HBM, FILLS[1], stream_map=chosen)
        case.check(dev, PS.HBM, only=set(chosen))


# ------------------------------------------------------------------ table -> KV -> pending
def test_table_then_kv_then_pending(gpu):
    batch = KS.table_batch(True)
    KS.check_precondition(batch)
    planes = ft.pack_table_streams([b[0] for b in batch], KS.N, KS.KEYS)
    ops, omax = K.pack_kv_ops([b[3] for b in batch], planes.steps, omax=2)
    S, steps = planes.S, planes.steps
    tab = fd.run_table(planes, KS.THR, keep_device=True, order_fill=0xA5)
    assert np.all(tab.err == 0)
    nkeys = fd.DeviceBuffer(planes.nkeys.nbytes)
    nkeys.upload(planes.nkeys)
    # the executor's outputs and its planes are read where they are
    kv = fd.run_kv(tab.dev["order"], tab.dev["nexec"], tab.dev["hdr"], ops, S, steps, KS.KEYS, omax,
                   key_mask=0x00FFFFFF, fill=0xA5)
    res = fd.run_pending(tab.dev["order"], tab.dev["nexec"], tab.dev["dot"], nkeys, S, steps, fill=0xA5,
                         before_launch=poisoner(*FILLS[1]))
    same_bytes(res, P.run_pending_host(tab.order, tab.nexec, planes.dot, planes.nkeys, S, steps, fill=0xA5))
    assert res.status == 0 and res.reruns == 0
    per_stream = []
    for s, (ev, ref, keys_of, ops_of) in enumerate(batch):
        want = pending_ref.run(ref["order"], [_lib.pack_dot(*e[2]) if e[0] == "A" else 0 for e in ev],
                               [(e[5] if len(e) > 5 else 1) if e[0] == "A" else 0 for e in ev], steps)
        assert res.ready_heads(s) == want["ready"] and int(res.nopen[s]) == 0
        assert int(res.nready[s]) == len({e[2] for e in ev if e[0] == "A"})
        for (j, h), a in want["part"].items():
            assert res.parts(s, h, j + 1)[j] == a
        per_stream.append(dict(P.command_results(res, kv, planes.hdr, s, key_mask=0x00FFFFFF, ops=ops)))
    for g in range(0, S, 4):
        assert all(per_stream[s] == per_stream[g] for s in range(g + 1, g + 4))


# ------------------------------------------------------------------ a closed-loop group -> pending
def test_behind_a_shard_group(gpu):
    """One group of 2 shards through fx_table_run_groups; the stage reads the group's order plane, whose
    arrival rows are handled rows, with the rifl and the count of every handled row gathered from the own
    rows handled_src names (a routed message is a row nobody waits for)."""
    shards, n, f = 2, 3, 1
    thr = T.quorum_sizes(n, f, False)[2]
    sts, commands, _ = TP.generated(shards, n, f, 10, count=1, per_shard=30)[0]
    own = TR.own_events(sts)
    planes, route, targets, steps_out = ft.pack_table_groups([(own, commands)], n, TP.KEYS)
    grp = fd.run_table_groups_packed(planes, route, targets, steps_out, shards, thr, fill=0xA5)
    streams, results = TR.closed_loop(own, commands, n, thr, TP.KEYS)
    S = shards
    pw = _lib.plane_words(S, steps_out)
    rifl, count = np.full(pw, PS.A5, np.uint32), np.full(pw, PS.A5, np.uint32)
    for s in range(S):
        L = int(grp.handled_len[s])
        rows = _lib.index(np.arange(L), s, steps_out)
        src = grp.handled_src[rows]
        msg = (src & _lib.FX_TABLE_HANDLED_MSG) != 0
        own_at = _lib.index(np.where(msg, 0, src), s, planes.steps)
        rifl[rows] = np.where(msg, grp.handled_dot[rows], planes.dot[own_at])
        count[rows] = np.where(msg, 0, planes.nkeys[own_at])
    res = fd.run_pending(grp.order, grp.nexec, rifl, count, S, steps_out, count_mask=0xFF, fill=0xA5,
                         before_launch=poisoner(*FILLS[2]))
    same_bytes(res, P.run_pending_host(grp.order, grp.nexec, rifl, count, S, steps_out, count_mask=0xFF, fill=0xA5))
    multi = 0
    for s in range(S):
        ev, ref = streams[s], results[s]
        assert ref["err"] == 0 == int(res.err[s])
        want = pending_ref.run(ref["order"], [_lib.pack_dot(*e[2]) if e[0] != "D" else 0 for e in ev],
                               [(e[5] if len(e) > 5 else 1) if e[0] == "A" else 0 for e in ev], steps_out)
        assert want["err"] == 0 and res.ready_heads(s) == want["ready"] and int(res.nopen[s]) == want["nopen"]
        rows = _lib.index(np.arange(len(ev)), s, steps_out)
        assert {a: int(h) for a, h in enumerate(res.head[rows]) if h != PS.A5} == want["head"]
        multi += sum(j > 0 for j, _ in want["part"])
    assert multi > 0


# ------------------------------------------------------------------ a generated batch
def test_device_streams_never_leave_the_device(gpu):
    """fx_table_synth_generate (kmax 2) -> fx_table_run_mk -> fx_pending_run over DeviceBuffers only."""
    p = ft.table_synth_params(seed=5, streams=65, n=5, fast_quorum=3, keys=16, cmds=30, conflicts=(2, 50), kmax=2,
                              stream_base=3)
    t = fd.synth_table(p)
    tab = fd.run_table(t, KS.THR, keep_device=True)
    assert np.all(tab.err == 0)
    res = fd.run_pending(tab.dev["order"], tab.dev["nexec"], t.bufs["dot"], t.nkeys, t.S, t.steps, fill=0xA5,
                         before_launch=poisoner(*FILLS[0]))
    host = t.download()
    same_bytes(res, P.run_pending_host(tab.order, tab.nexec, host.dot, host.nkeys, t.S, t.steps, fill=0xA5))
    assert res.status == 0 and np.all(res.err == 0) and int(res.nready.sum()) > 0
    for s in (0, 63, 64):
        rows = _lib.index(np.arange(t.steps), s, t.steps)
        order = [int(x) & 0x7FFFFFFF for x in tab.order[_lib.index(np.arange(int(tab.nexec[s])), s, t.steps)]]
        want = pending_ref.run(order, [int(x) for x in host.dot[rows]], [int(x) for x in host.nkeys[rows]], t.steps)
        assert want["err"] == 0 and res.ready_heads(s) == want["ready"] and int(res.nopen[s]) == want["nopen"]
        assert any(j == 1 for j, _ in want["part"])
