"""fx_table_run_groups on the GPU: the closed loop of a group of shard
executors inside one kernel launch (fantoch_amd.device.run_table_groups)
against the closed loop restated on the CPU (tests/table_resume.py), bit for
bit: the streams as handled, every field of the results, the rounds.  Every
error below is a per-stream status of a well-formed launch."""
import copy

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import table as ft

import table_ref_ps as RP
import table_resume as TR
import table_shapes as T
import table_shapes_ps as TP

pytestmark = pytest.mark.gpu

BAD, CAPACITY = _lib.FX_ERR_INVALID_ARG, _lib.FX_ERR_CAPACITY
HBM = _lib.FX_TABLE_TIER_HBM
NONE = _lib.FX_RELEASE_NONE
X, Y, Z, S1 = TP.X, TP.Y, TP.Z, TP.S1


def spread_delay(sender, dot, target, key):
    """0..31 rounds."""
    return (7 * dot[1] + key) % 32


def trace(own, commands, n, thr, keys, delay=None):
    """TR.closed_loop again, keeping what it forgets: the messages as (round
    sent, due round, send index, target shard), the most undelivered messages
    a shard held and the most sends of a shard in one round."""
    G = len(own)
    sims = [RP.Stream(n, thr, keys) for _ in range(G)]
    streams, due, msgs = [[] for _ in range(G)], [[] for _ in range(G)], []
    nsent = t = most_due = most_sends = 0
    while any(sims[g].err == 0 and (t < len(own[g]) or due[g]) for g in range(G)):
        for g in range(G):
            if sims[g].err:
                due[g] = []
                continue
            now = sorted(m for m in due[g] if m[0] <= t)
            due[g] = [m for m in due[g] if m[0] > t]
            sends = 0
            for ev in [("S", x, dot) for _, _, x, dot in now] + ([own[g][t]] if t < len(own[g]) else []):
                before = set(sims[g].ex.sent)
                streams[g].append(ev)
                if sims[g].err == 0:
                    sims[g].feed(ev)
                for a in sorted(set(sims[g].ex.sent) - before):
                    dot = streams[g][a][2]
                    sends += len(commands[dot]) > 1
                    for h in sorted(commands[dot]):
                        if h != g:
                            for x in sorted(commands[dot][h]):
                                lag = delay(g, dot, h, x) if delay else 0
                                due[h].append((t + 1 + lag, nsent, x, dot))
                                msgs.append((t, t + 1 + lag, nsent, h))
                                nsent += 1
            most_sends = max(most_sends, sends)
        most_due = max([most_due] + [len(due[g]) for g in range(G) if sims[g].err == 0])
        t += 1
    assert (streams, [s.result() for s in sims]) == TR.closed_loop(own, commands, n, thr, keys, delay)
    return dict(streams=streams, results=[s.result() for s in sims], rounds=t, msgs=msgs, most_due=most_due,
                most_sends=most_sends)


def overtaken(msgs):
    """A message sent later (a higher send index) and due earlier than another to the same shard."""
    return any(a[3] == b[3] and a[2] < b[2] and b[1] < a[1] for a in msgs for b in msgs)


def same(got, want):
    """One group: the streams as handled, every field of every shard's result, the rounds."""
    assert got["streams"] == want["streams"]
    for g, (r, w) in enumerate(zip(got["results"], want["results"])):
        for f in TR.FIELDS:
            assert r[f] == w[f], (g, f)
    assert got["rounds"] == want["rounds"]


def run_whole(streams, results, n, thr, keys):
    """The streams as handled, run whole through the _ps entry points, give the same rows."""
    planes = ft.pack_table_streams(streams, n, keys)
    res = fd.run_table(planes, thr, shards=True)
    for s, ref in enumerate(results):
        assert res.err[s] == ref["err"] and res.nexec[s] == ref["nexec"], s
        rows = _lib.index(np.arange(ref["nexec"]), s, planes.steps)
        assert [int(x) & ~_lib.FX_ORDER_SCC_START for x in res.order[rows]] == ref["order"], s
        for name, plane in (("release", res.release), ("sent", res.stable_sent)):
            got = plane[_lib.index(np.arange(len(streams[s])), s, planes.steps)]
            assert {a: int(v) for a, v in enumerate(got) if v != NONE} == ref[name], (s, name)
        assert list(res.stable_clock[s]) == ref["stable"], s


def check_groups(groups, n, thr, keys, delay=None, whole=True):
    out = fd.run_table_groups(groups, n, keys, thr, delay=delay)
    wants = [trace(own, commands, n, thr, keys, delay) for own, commands in groups]
    for got, want in zip(out, wants):
        same(got, want)
    if whole:
        run_whole([st for got in out for st in got["streams"]], [r for got in out for r in got["results"]], n, thr,
                  keys)
    return out, wants


# ------------------------------------------------------ 1. generated groups
@pytest.mark.parametrize("delay", [None, TR.hashed_delay, spread_delay], ids=["next", "hashed", "spread"])
@pytest.mark.parametrize("shards,n,f", TP.GROUPS)
def test_generated_groups(shards, n, f, delay):
    """The first two seeds of both conflict rates, and one group cut short so
    that the workgroups of the launch run different numbers of rounds."""
    thr = T.quorum_sizes(n, f, False)[2]
    groups = [(TR.own_events(sts), commands) for c in TP.CONFLICTS
              for sts, commands, _ in TP.generated(shards, n, f, c, msg_lag=0)[:2]]
    own, commands = groups[1]
    groups.append(([o[:len(o) // 3] for o in own], commands))
    out, wants = check_groups(groups, n, thr, TP.KEYS, delay)
    assert len({w["rounds"] for w in wants}) > 1
    assert sum(len(r["sent"]) for w in wants for r in w["results"]) > 100
    assert all(r["err"] == 0 for w in wants for r in w["results"])
    if delay is not None:
        assert any(overtaken(w["msgs"]) for w in wants)


# ---------------------------------------------- 2. eight shards, one shard
@pytest.mark.parametrize("conflict", TP.CONFLICTS)
def test_eight_shards(conflict):
    """The full workgroup."""
    thr = T.quorum_sizes(5, 1, False)[2]
    groups = [(TR.own_events(sts), commands)
              for sts, commands, _ in TP.generated(8, 5, 1, conflict, per_shard=20, count=2)]
    out, wants = check_groups(groups, 5, thr, TP.KEYS, TR.hashed_delay)
    assert all(len(own) == 8 and all(own) for own, _ in groups)
    assert sum(ev[0] == "S" for w in wants for st in w["streams"] for ev in st) > 50


def test_one_shard_is_run_ps():
    """P = 1: nothing to route; every stream against fx_table_execute_ps at the HBM tier."""
    n, fq, _, thr = (5,) + T.quorum_sizes(5, 1, False)
    streams = [ft.synth_table_streams_mk(seed, n, fq, TP.KEYS, 40 + 7 * seed, 50, 4, 2, 3) for seed in range(5)]
    groups = [([st], {}) for st in streams]
    out = fd.run_table_groups(groups, n, TP.KEYS, thr)
    planes = ft.pack_table_streams(streams, n, TP.KEYS)
    res = fd.run_table(planes, thr, tier=HBM, multi=True, shards=True)
    for s, got in enumerate(out):
        r = got["results"][0]
        assert got["streams"] == [streams[s]] and got["rounds"] == len(streams[s])
        assert r["err"] == res.err[s] == 0 and r["nexec"] == res.nexec[s] > 0
        rows = _lib.index(np.arange(len(streams[s])), s, planes.steps)
        assert r["order"] == [int(x) & ~_lib.FX_ORDER_SCC_START for x in res.order[rows[:r["nexec"]]]]
        for name, plane in (("release", res.release), ("sent", res.stable_sent)):
            assert r[name] == {a: int(v) for a, v in enumerate(plane[rows]) if v != NONE}, name
        assert len(r["sent"]) > 0 and r["stable"] == list(res.stable_clock[s])


# ------------------------------------------------------------ 3. hand cases
def no_votes(key, dot, clock, nkeys, shards):
    return ("A", key, dot, clock, [], nkeys, shards)


def hand(own, commands, delay=None, keys=TP.HAND_KEYS):
    (got,), (want,) = check_groups([(own, commands)], TP.HAND_N, TP.HAND_THR, keys, delay)
    return want


def test_sends_of_one_step_go_out_in_row_order():
    """Shard 0, key 0: X (two keys here) waits at the head, Z behind it.  The
    event that makes X stable here (row 4) sends X, the drain of the same step
    executes X's op on key 0 and the queue runs on to Z (row 0), which sends
    too: tried X then Z, routed Z then X."""
    own = [[no_votes(0, Z, 2, 1, 2), ("A", 0, X, 1, [(1, 1, 2), (2, 1, 2)], 2, 2), TP.att(1, X, 1, 1, 2, 2)],
           [TP.att(0, X, 1, 1, 1, 2)]]
    commands = {X: {0: [0, 1], 1: [0]}, Z: {0: [0], 1: [2]}}
    want = hand(own, commands)
    assert want["results"][0]["sent"] == {0: 4, 4: 4}  # one step, rows 0 and 4
    assert want["results"][0]["order"] == [4, 3]       # X's partials executed in that step, before Z was tried
    assert want["streams"][1] == [own[1][0], ("S", 2, Z), ("S", 0, X)]
    # a message due after its target's last own event
    assert [m[1] for m in want["msgs"] if m[3] == 1] == [3, 3] and len(own[1]) == 1


def test_a_shard_without_own_events():
    own = [[TP.att(0, X, 1, 1, 1, 2)], [TP.att(0, S1, 1, 1, 1, 1)], []]
    want = hand(own, {X: {0: [0], 2: [1]}, S1: {1: [0]}}, TR.hashed_delay)
    assert want["streams"][2] == [("S", 1, X)] and want["results"][2]["nexec"] == 0
    assert want["results"][1]["order"] == [0]


def test_a_message_for_an_op_in_the_votes_table():
    own = [[TP.att(0, X, 1, 1, 1, 2)], [no_votes(1, X, 1, 1, 2), ("D", 1, [(1, 1, 1), (2, 1, 1)])]]
    want = hand(own, {X: {0: [0], 1: [1]}})
    assert want["streams"][1] == [own[1][0], ("S", 1, X), own[1][1]]
    sim = RP.Stream(TP.HAND_N, TP.HAND_THR, TP.HAND_KEYS)
    for ev in want["streams"][1][:2]:
        sim.feed(ev)
    assert sim.ex.npairs == 1 and TR.op_states(sim.ex) == {"table"}  # buffered, the op not yet stable
    assert want["results"][1]["release"] == {0: 2} and want["results"][0]["release"] == {0: 1}


def test_execute_at_commit():
    """Attached events execute at their own step and nothing is sent."""
    thr = T.quorum_sizes(3, 1, False)[2]
    sts, commands, _ = TP.generated(3, 3, 1, 100, msg_lag=0)[0]
    own = TR.own_events(sts)
    (got,) = fd.run_table_groups([(own, commands)], 3, TP.KEYS, thr, delay=TR.hashed_delay, execute_at_commit=True)
    assert got["streams"] == own and got["rounds"] == max(len(o) for o in own)
    for o, r in zip(own, got["results"]):
        ref = RP.run_stream(list(o), 3, thr, TP.KEYS, execute_at_commit=True)
        assert ref["sent"] == {} and ref["nexec"] > 0
        assert all(r[f] == ref[f] for f in TR.FIELDS)


# --------------------------------------------------------- 4. a shard stops
def stop_group():
    """The shape of stop_group in tests/test_table_resume_gpu.py: shard 1 stops
    with FX_ERR_INVALID_ARG at its third event, before shard 0's message to it
    is due.  (There the failing stream holds "S" events of its own, which a
    group's own events cannot: here an attached event with no keys.)"""
    own = [[TP.att(0, S1, 1, 1, 1, 1), ("D", 0, [(3, 1, 1)]), ("D", 2, [(3, 1, 1)]), ("D", 2, [(3, 2, 2)]),
            TP.att(1, Y, 2, 1, 1, 2)],
           [TP.att(1, S1, 1, 1, 1, 1), ("D", 2, [(3, 1, 1)]), TP.att(0, X, 1, 1, 0, 1), ("D", 2, [(3, 2, 2)])]]
    return own, {Y: {0: [1], 1: [2]}}


def test_a_shard_stops_mid_stream():
    own, commands = stop_group()
    thr = T.quorum_sizes(3, 1, False)[2]
    other = TP.generated(2, 3, 1, 10, msg_lag=0)[0]
    groups = [(own, commands), (TR.own_events(other[0]), other[1])]
    out, wants = check_groups(groups, 3, thr, TP.KEYS, whole=False)
    want = wants[0]
    assert want["results"][1]["err"] == BAD and want["results"][0]["err"] == 0
    assert want["streams"][1] == own[1][:3]  # its last handled row is the failing event
    assert want["results"][0]["sent"] == {4: 4} and want["rounds"] == 5  # the message to it vanished
    assert len(want["msgs"]) == 1


# ----------------------------------------------------------- 5. capacities
def inbox_group(last):
    """Shard 0 sends in each of 32 rounds one command's messages, 8 keys at
    shard 1 (the last command: `last` keys), each due 32 rounds later: after
    round 31 shard 1 holds 248 + last undelivered messages."""
    own = [[TP.att(i, (1, i + 1), 1, 1, 1, 2) for i in range(32)], []]
    commands = {(1, i + 1): {0: [i], 1: list(range(8 if i < 31 else last))} for i in range(32)}
    return own, commands


def test_inbox_capacity():
    slow = lambda g, dot, t, x: 31
    thr, keys = TP.HAND_THR, 40
    own, commands = inbox_group(8)
    (got,), (want,) = check_groups([(own, commands)], TP.HAND_N, thr, keys, slow, whole=False)
    assert want["most_due"] == _lib.FX_TABLE_GROUP_INBOX == 256 and len(want["streams"][1]) == 256
    own, commands = inbox_group(9)
    want = trace(own, commands, TP.HAND_N, thr, keys, slow)
    assert want["most_due"] == 257 and want["msgs"][-1][0] == 31
    (got,) = fd.run_table_groups([(own, commands)], TP.HAND_N, keys, thr, delay=slow)
    # shard 1 stops in round 31, before it handled anything; shard 0 finishes
    assert got["results"][1]["err"] == CAPACITY and got["streams"][1] == [] and got["results"][1]["nexec"] == 0
    assert got["streams"][0] == want["streams"][0] and got["rounds"] == 32
    assert all(got["results"][0][f] == want["results"][0][f] for f in TR.FIELDS)


def sends_group(count):
    """Shard 1 tells shard 0 of `count` commands, one a round; at shard 0 they
    wait in key 0's votes table, the messages are buffered, and one detached
    event makes all of them stable: `count` tries in one step, each sends and
    executes."""
    dots = [(1, i + 1) for i in range(count)]
    own = [[no_votes(0, d, i + 1, 1, 2) for i, d in enumerate(dots)] + [("D", 0, [(1, 1, count), (2, 1, count)])],
           [TP.att(i, d, i + 1, 1, 1, 2) for i, d in enumerate(dots)]]
    return own, {d: {0: [0], 1: [i]} for i, d in enumerate(dots)}


def test_sends_capacity():
    thr, keys = TP.HAND_THR, 72
    own, commands = sends_group(64)
    (got,), (want,) = check_groups([(own, commands)], TP.HAND_N, thr, keys, whole=False)
    assert want["most_sends"] == _lib.FX_TABLE_GROUP_SENDS == 64
    assert want["results"][0]["nexec"] == want["results"][1]["nexec"] == 64
    own, commands = sends_group(65)
    want = trace(own, commands, TP.HAND_N, thr, keys)
    assert want["most_sends"] == 65 and len(want["streams"][0]) == 131
    (got,) = fd.run_table_groups([(own, commands)], TP.HAND_N, keys, thr)
    r0, r1 = got["results"]
    # shard 0 stops at its last event, row 130, at the 65th try; the 64 before it were sent and routed
    assert r0["err"] == CAPACITY and got["streams"][0] == want["streams"][0] and r0["nexec"] == 64
    assert r0["sent"] == {a: 130 for a in range(0, 128, 2)} and r0["order"] == list(range(0, 128, 2))
    assert r1["err"] == 0 and r1["nexec"] == 64 and len(got["streams"][1]) == 65 + 64


# ---------------------------------------------------------- 6. input check
def check_group():
    own = [[TP.att(0, X, 1, 1, 2, 2), TP.att(1, X, 1, 1, 2, 2), TP.att(2, S1, 1, 1, 1, 1), TP.att(2, Y, 2, 2, 1, 2)],
           [TP.att(1, Y, 1, 1, 1, 2), ("D", 0, [(3, 1, 1)]), TP.att(0, X, 2, 2, 1, 2)]]
    return own, {X: {0: [0, 1], 1: [0]}, Y: {0: [2], 1: [1]}, S1: {0: [2]}}


BAD_INPUTS = ["route_none", "own_shard", "shard_p", "key_keys", "last_word", "s_event"]


@pytest.mark.parametrize("what", BAD_INPUTS)
def test_input_check(what):
    """Each bad value stops its stream before round 0 and no other.  The
    targets buffer is 64 words longer than targets_words says."""
    groups = [check_group(), check_group()]
    planes, route, targets, steps_out = ft.pack_table_groups(groups, TP.HAND_N, TP.HAND_KEYS)
    words = len(targets)
    targets = np.concatenate([targets, np.zeros(64, np.uint32)])
    s, row = 2, 0  # group 1, shard 0, X's first event
    at = int(_lib.index(row, s, planes.steps))
    rt = int(route[at])
    assert rt != _lib.FX_TABLE_ROUTE_NONE and targets[rt] == 1
    planes = copy.copy(planes)
    planes.hdr = planes.hdr.copy()
    if what == "route_none":
        route[at] = _lib.FX_TABLE_ROUTE_NONE
    elif what == "own_shard":
        targets[rt + 1] = ft.table_target(0, 0, 0)
    elif what == "shard_p":
        targets[rt + 1] = ft.table_target(0, 2, 0)
    elif what == "key_keys":
        targets[rt + 1] = ft.table_target(0, 1, TP.HAND_KEYS)
    elif what == "last_word":
        route[at] = words - 1
    else:
        planes.hdr[at] = ft.table_hdr_stable(0)
    res = fd.run_table_groups_packed(planes, route, targets, steps_out, 2, TP.HAND_THR, targets_words=words)
    assert res.err.tolist() == [0, 0, BAD, 0]
    assert res.nexec[s] == 0 and res.handled_len[s] == 0
    # the group of the good streams is the closed loop; the stopped stream's neighbour went on alone
    good = fd.table_group_dicts(groups, res)
    same(good[0], trace(*groups[0], TP.HAND_N, TP.HAND_THR, TP.HAND_KEYS))
    assert good[1]["streams"][1] == groups[1][0][1] and res.rounds[1] == 3


# --------------------------------------------------------------- 7. poison
def test_poisoned_buffers():
    """`state`, every output and the input rows at and above each stream's
    length start as 0xA5 bytes: nothing changes."""
    n, thr = 3, T.quorum_sizes(3, 1, False)[2]
    groups = [(TR.own_events(sts), commands) for sts, commands, _ in TP.generated(3, 3, 1, 100, msg_lag=0)[:2]]
    own, commands = groups[1]
    groups.append(([o[:len(o) // 2] for o in own], commands))
    planes, route, targets, steps_out = ft.pack_table_groups(groups, n, TP.KEYS, TR.hashed_delay)
    clean = fd.table_group_dicts(groups, fd.run_table_groups_packed(planes, route, targets, steps_out, 3, thr, fill=0))
    keep = np.concatenate([_lib.index(np.arange(int(l)), s, planes.steps) for s, l in enumerate(planes.lengths)])
    dirty = copy.copy(planes)
    for name in ("hdr", "dot", "clock", "nkeys"):
        arr = np.full(planes.plane, 0xA5A5A5A5, np.uint32)
        arr[keep] = getattr(planes, name)[keep]
        setattr(dirty, name, arr)
    dirty.votes = np.full(planes.votes.size, 0xA5A5A5A5, np.uint32)
    for p in range(3 * planes.vmax):
        dirty.votes[p * planes.plane + keep] = planes.votes[p * planes.plane + keep]
    bad_route = np.full(planes.plane, 0xA5A5A5A5, np.uint32)
    bad_route[keep] = route[keep]
    got = fd.table_group_dicts(groups, fd.run_table_groups_packed(dirty, bad_route, targets, steps_out, 3, thr,
                                                                  fill=0xA5))
    assert got == clean
    for g, (o, c) in zip(got, groups):
        same(g, trace(o, c, n, thr, TP.KEYS, TR.hashed_delay))


# ------------------------------------------------------- 8. the round cap
def test_the_cap_on_rounds():
    """A cap of 3 rounds on groups that need many more: the call returns and
    every stream reports FX_ERR_INVALID_ARG with what it handled in 3 rounds."""
    n, thr = 3, T.quorum_sizes(3, 1, False)[2]
    groups = [(TR.own_events(sts), commands) for sts, commands, _ in TP.generated(2, 3, 1, 10, msg_lag=0)[:2]]
    planes, route, targets, steps_out = ft.pack_table_groups(groups, n, TP.KEYS)
    out = fd.table_group_dicts(groups, fd.run_table_groups_packed(planes, route, targets, steps_out, 2, thr,
                                                                  max_rounds=3))
    for got, (own, commands) in zip(out, groups):
        assert min(len(o) for o in own) > 3 and got["rounds"] == 3
        assert [r["err"] for r in got["results"]] == [BAD, BAD]
        for st, o in zip(got["streams"], own):
            assert TR.own_events([st])[0] == o[:3]
