"""fx_table_run_groups without a GPU: the packer (routes and target lists),
the rebuild of the handled streams, the C ABI (struct layouts against the
header, argument checks) and the cap on rounds the host computes.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import table as ft

import table_resume as TR
import table_shapes as T
import table_shapes_ps as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSG = _lib.FX_TABLE_HANDLED_MSG


def hand_group():
    """Two shards, three commands: X on both (two keys at shard 0), Y on both, S1 at shard 0 only."""
    own = [[TP.att(0, TP.X, 1, 1, 2, 2), TP.att(1, TP.X, 1, 1, 2, 2), TP.att(2, TP.S1, 1, 1, 1, 1),
            TP.att(2, TP.Y, 2, 2, 1, 2)],
           [TP.att(1, TP.Y, 1, 1, 1, 2), ("D", 0, [(3, 1, 1)]), TP.att(0, TP.X, 2, 2, 1, 2)]]
    return own, {TP.X: {0: [0, 1], 1: [0]}, TP.Y: {0: [2], 1: [1]}, TP.S1: {0: [2]}}


def lists_of(planes, route, targets, s):
    """Per own row of stream s: None, or the (delay, shard, key) tuples its route points at."""
    out = []
    for r in range(int(planes.lengths[s])):
        rt = int(route[int(_lib.index(r, s, planes.steps))])
        if rt == _lib.FX_TABLE_ROUTE_NONE:
            out.append(None)
            continue
        m = int(targets[rt])
        out.append((rt, [(int(w) >> 27, (int(w) >> 24) & 7, int(w) & 0xFFFFFF) for w in targets[rt + 1:rt + 1 + m]]))
    return out


def check_packing(groups, keys, n, delay):
    planes, route, targets, steps_out = ft.pack_table_groups(groups, n, keys, delay)
    P = len(groups[0][0])
    assert planes.S == len(groups) * P and planes.ps
    assert steps_out == ft.group_steps_out(groups)
    routed = 0
    for i, (own, commands) in enumerate(groups):
        for h in range(P):
            s = i * P + h
            assert planes.stream(s) == ft.pack_table_streams([own[h], [TP.st(0, TP.X)]], n, keys).stream(0)
            by_dot = {}
            for ev, got in zip(own[h], lists_of(planes, route, targets, s)):
                if ev[0] != "A" or len(ev) != 7 or ev[6] == 1:
                    assert got is None
                    continue
                want = [((delay(h, ev[2], t, x) if delay else 0), t, x)
                        for t, x, _, _ in ft.stable_messages([(ev[2], 0)], commands, h)]
                assert got[1] == want and len(want) >= 1
                assert by_dot.setdefault(ev[2], got[0]) == got[0]  # one list per command and shard
                routed += 1
    return routed, targets


def test_packing_of_a_hand_group():
    own, commands = hand_group()
    routed, targets = check_packing([(own, commands)], TP.HAND_KEYS, TP.HAND_N, TR.hashed_delay)
    assert routed == 5
    # X at shard 0 (one list for its two events), Y at shard 0, Y at shard 1, X at shard 1 (two keys)
    assert len(targets) == 2 + 2 + 2 + 3
    assert ft.group_steps_out([(own, commands)]) == max(4 + 2 + 1, 3 + 1 + 1)


def test_packing_of_generated_groups():
    n, thr = 5, T.quorum_sizes(5, 1, False)[2]
    groups = [(TR.own_events(sts), commands) for sts, commands, _ in TP.generated(3, 5, 1, 100, msg_lag=0)[:2]]
    routed, _ = check_packing(groups, TP.KEYS, n, lambda g, dot, t, x: (7 * dot[1] + x) % 32)
    assert routed > 50


def test_packer_refuses():
    own, commands = hand_group()
    with pytest.raises(ValueError):
        ft.pack_table_groups([(own, commands)], TP.HAND_N, TP.HAND_KEYS, lambda *a: 32)
    ft.pack_table_groups([(own, commands)], TP.HAND_N, TP.HAND_KEYS, lambda *a: 31)
    with pytest.raises(ValueError):
        ft.pack_table_groups([(own, commands), (own + [[]], commands)], TP.HAND_N, TP.HAND_KEYS)
    with pytest.raises(ValueError):  # a command the map does not have at this shard
        ft.pack_table_groups([(own, {TP.X: commands[TP.X], TP.S1: commands[TP.S1]})], TP.HAND_N, TP.HAND_KEYS)


def handled_planes(own, streams):
    """What the kernel writes into handled_src / handled_dot for these streams."""
    out = []
    for o, st in zip(own, streams):
        src, dot, r = [], [], 0
        for ev in st:
            if ev[0] == "S":
                src.append(MSG | ev[1])
                dot.append(_lib.pack_dot(*ev[2]))
            else:
                assert ev == o[r]
                src.append(r)
                dot.append(0)
                r += 1
        out.append((np.array(src, np.uint32), np.array(dot, np.uint32)))
    return out


@pytest.mark.parametrize("delay", [None, TR.hashed_delay])
def test_rebuilding_the_handled_streams(delay):
    n, thr = 3, T.quorum_sizes(3, 1, False)[2]
    sts, commands, _ = TP.generated(3, 3, 1, 100, msg_lag=0)[0]
    own = TR.own_events(sts)
    streams, _ = TR.closed_loop(own, commands, n, thr, TP.KEYS, delay)
    assert sum(ev[0] == "S" for st in streams for ev in st) > 20
    for o, st, (src, dot) in zip(own, streams, handled_planes(own, streams)):
        assert ft.handled_stream(o, src, dot) == st
    assert max(len(st) for st in streams) <= ft.group_steps_out([(own, commands)])


# ------------------------------------------------------------------ C ABI
PAIRS = {"TableGroupBatch": "fx_table_group_batch", "TableGroupOut": "fx_table_group_out"}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ctypes_mirrors_match_the_header():
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "fantoch_amd.h"', "int main(void) {"]
    for py, c in PAIRS.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (py, c))
        for name, _ in getattr(_lib, py)._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (py, name, c, name))
    lines.append('  printf("T target %u\\n", (unsigned)FX_TABLE_TARGET(31u, 7u, 0xABCDEFu));')
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
    layout = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out.split("\n") if ln}
    for py in PAIRS:
        cls = getattr(_lib, py)
        assert ctypes.sizeof(cls) == layout[(py, "size")], py
        for name, _ in cls._fields_:
            assert getattr(cls, name).offset == layout[(py, name)], (py, name)
    assert layout[("T", "target")] == ft.table_target(31, 7, 0xABCDEF)


def test_symbols_and_constants(lib):
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for name in ("fx_table_groups_state_bytes", "fx_table_run_groups", "fx_table_run_groups_capped"):
        assert hasattr(lib, name) and name in bound
    text = open(os.path.join(ROOT, "include", "fantoch_amd.h")).read()
    for name in ("FX_TABLE_GROUP_MAX_DELAY", "FX_TABLE_GROUP_INBOX", "FX_TABLE_GROUP_SENDS"):
        assert int(re.search(r"#define %s (\d+)u" % name, text).group(1)) == getattr(_lib, name)
    for name in ("FX_TABLE_ROUTE_NONE", "FX_TABLE_HANDLED_MSG"):
        assert int(re.search(r"#define %s (0x[0-9A-F]+)u" % name, text).group(1), 16) == getattr(_lib, name)
    assert int(re.search(r"#define FX_PROFILE_SLOTS (\d+)u", text).group(1)) > _lib.FX_PROFILE_SLOT_TABLE + 3
    assert lib.fx_table_groups_state_bytes(5, 16, 6) == lib.fx_table_state_bytes_ps(5, 16, 6)


def call(lib, null=None, flags=0, shards=2, S=4, steps=8, steps_out=12, n=3, thr=2, keys=4, capped=None):
    """fx_table_run_groups over host arrays (no launch happens without a device)."""
    pw, ow = _lib.plane_words(S, steps), _lib.plane_words(S, steps_out)
    arr = {nm: np.zeros(pw, np.uint32) for nm in ("hdr", "dot", "clock", "nkeys", "route")}
    arr["votes"] = np.zeros(3 * pw, np.uint32)
    arr["targets"] = np.zeros(16, np.uint32)
    arr.update({nm: np.zeros(ow, np.uint32) for nm in ("order", "release", "sent", "hsrc", "hdot")})
    arr.update({nm: np.zeros(max(S, 1), np.uint32) for nm in ("nexec", "err", "hlen", "rounds", "stable")})
    arr["state"] = np.zeros(max(lib.fx_table_groups_state_bytes(n, max(keys, 1), S), 4) // 4, np.uint32)
    ptr = lambda nm: None if null == nm else arr[nm].ctypes.data
    base = _lib.TableBatch(ptr("hdr"), ptr("dot"), ptr("clock"), ptr("votes"), None, S, steps, n, keys, 1, thr)
    inb = _lib.TableGroupBatch(_lib.TableBatchMk(base, ptr("nkeys")), ptr("route"), ptr("targets"), 16, shards,
                               steps_out)
    outb = _lib.TableGroupOut(_lib.OrderBatch(ptr("order"), ptr("release"), ptr("nexec"), ptr("err")),
                              None, ptr("sent"), ptr("hsrc"), ptr("hdot"), ptr("hlen"),
                              ptr("rounds"))
    args = (None if null == "in" else ctypes.byref(inb), None if null == "out" else ctypes.byref(outb), ptr("state"),
            flags, None)
    return lib.fx_table_run_groups(*args) if capped is None else lib.fx_table_run_groups_capped(*args, capped)


def test_argument_checks_come_before_the_device_check(lib):
    bad = _lib.FX_ERR_INVALID_ARG
    for null in ("in", "out", "state", "hdr", "dot", "clock", "votes", "nkeys", "route", "targets", "order", "release",
                 "nexec", "err", "sent", "hsrc", "hdot", "hlen", "rounds"):
        assert call(lib, null=null) == bad, null
    for flags in (_lib.FX_FLAG_INIT, 4, 1 << 8):
        assert call(lib, flags=flags) == bad
    assert call(lib, shards=0) == bad and call(lib, shards=9) == bad
    assert call(lib, shards=3) == bad  # 4 streams
    assert call(lib, steps_out=0) == bad and call(lib, steps_out=1 << 26) == bad
    assert call(lib, steps=1 << 26) == bad and call(lib, steps=0) == bad
    assert call(lib, n=17) == bad and call(lib, thr=4) == bad and call(lib, thr=0) == bad and call(lib, keys=0) == bad
    assert call(lib, null="rounds", capped=3) == bad


def test_well_formed_calls_reach_the_device_check(lib):
    want = _lib.FX_ERR_NO_DEVICE if lib.fx_device_count() <= 0 else _lib.FX_OK
    if want == _lib.FX_OK:
        pytest.skip("a GPU is visible: the GPU tests make these calls")
    assert call(lib) == want and call(lib, flags=_lib.FX_FLAG_EXECUTE_AT_COMMIT) == want
    assert call(lib, shards=1) == want and call(lib, shards=4) == want and call(lib, capped=3) == want
    assert call(lib, S=8, shards=8) == want


# --------------------------------------------------------- the cap on rounds
def test_the_cap_on_rounds_holds_for_the_closed_loop():
    """The library caps a call at own.steps + 33 * shards * steps_out + 1 rounds.
    On the restatement: a group runs no longer than its longest own stream plus
    33 rounds per message handled, so never as long as that."""
    slow = lambda g, dot, t, x: 31
    for shards, n, f in TP.GROUPS:
        thr = T.quorum_sizes(n, f, False)[2]
        sts, commands, _ = TP.generated(shards, n, f, 100, msg_lag=0)[0]
        own = TR.own_events(sts)
        streams, _ = TR.closed_loop(own, commands, n, thr, TP.KEYS, slow)
        rounds = run_rounds(own, commands, n, thr, slow)
        msgs = sum(ev[0] == "S" for st in streams for ev in st)
        steps, steps_out = max(len(o) for o in own), ft.group_steps_out([(own, commands)])
        assert max(len(st) for st in streams) <= steps_out
        assert rounds <= steps + 33 * msgs + 1 <= steps + 33 * shards * steps_out + 1


def run_rounds(own, commands, n, thr, delay):
    """The rounds of closed_loop: run_table_groups over the restatement counts them."""
    out = ft.run_table_groups([(own, commands)], n, TP.KEYS, thr, delay=delay, session=TR.RefSession)[0]
    return out["rounds"]
