"""The argument checks of the graph, predecessors and pending entry points, one
table over fx_batch_execute, fx_batch_execute_partial, fx_batch_run_tiered,
fx_pred_execute, fx_pred_run, fx_pending_aggregate and fx_pending_run, in the
manner of tests/test_table_args_cpu.py: one valid argument set per entry point
over poison integers for pointers, then one mutation per row.  A row of
MUTATIONS is refused with FX_ERR_INVALID_ARG before the library looks for a
device.  A row of LATE is checked after the device: FX_ERR_NO_DEVICE without
one, FX_ERR_INVALID_ARG -- before anything is launched -- with one.  The
drivers write *reruns = 0 before any check and leave tier_counts alone on a
refusal.  CPU only."""
import ctypes

import pytest

from fantoch_amd import _lib

INIT, AT_COMMIT, SAVE, PARTIAL = _lib.FX_FLAG_INIT, _lib.FX_FLAG_EXECUTE_AT_COMMIT, _lib.FX_FLAG_SAVE_STATE, 8
GROUP, GLOBAL, SPLIT, WIDE, WIDE_HBM = _lib.FX_TIER_GROUP, 2, _lib.FX_TIER_SPLIT, _lib.FX_TIER_WIDE, _lib.FX_TIER_WIDE_HBM
PRED_MAX_DEPS = 256

NAMES = ("dot", "hdr", "deps", "clock_lo", "clock_hi", "ndeps", "order", "release", "nexec", "err", "map", "state",
         "frontier", "req", "rifl", "count", "p_order", "p_nexec", "part", "head", "ready", "index", "nready", "nopen",
         "p_err")
POISON = {name: 0x5A5A0000 + 64 * i for i, name in enumerate(NAMES)}  # never dereferenced

VALID = dict(null=None, n=3, dmax=2, steps=8, S=4, flags=INIT, tier=0, state=False, map=False, lanes=4, begin=0, end=8,
             req_cap=16, ndeps=True, count_mask=0xFF)


def ptr(a, name):
    return None if a["null"] == name else POISON[name]


def ref(a, name, obj):
    return None if a["null"] == name else ctypes.byref(obj)


def streams(a):
    return _lib.StreamBatch(ptr(a, "dot"), ptr(a, "hdr"), ptr(a, "deps"), None, a["S"], a["steps"], a["dmax"], a["n"])


def pred(a):
    return _lib.PredBatch(streams(a), ptr(a, "clock_lo"), ptr(a, "clock_hi"), POISON["ndeps"] if a["ndeps"] else None)


def order(a):
    return _lib.OrderBatch(ptr(a, "order"), ptr(a, "release"), ptr(a, "nexec"), ptr(a, "err"))


def pending_in(a):
    return _lib.PendingBatch(ptr(a, "p_order"), ptr(a, "p_nexec"), ptr(a, "rifl"), ptr(a, "count"), a["count_mask"], 0,
                             a["S"], a["steps"])


def pending_out(a):
    return _lib.PendingOut(ptr(a, "part"), ptr(a, "head"), ptr(a, "ready"), ptr(a, "index"), ptr(a, "nready"),
                           ptr(a, "nopen"), ptr(a, "p_err"))


def opt(a, name):
    return POISON[name] if a[name] else None


def execute(lib, a):
    return lib.fx_batch_execute(ref(a, "in", streams(a)), ref(a, "out", order(a)), a["tier"], opt(a, "map"),
                                a["lanes"], opt(a, "state"), a["begin"], a["end"], a["flags"], None, None)


def partial(lib, a):
    return lib.fx_batch_execute_partial(ref(a, "in", streams(a)), ref(a, "out", order(a)), ptr(a, "state"), a["begin"],
                                        a["end"], a["flags"], POISON["frontier"], ptr(a, "req"), a["req_cap"], None)


def run_tiered(lib, a):
    counts = (ctypes.c_uint32 * _lib.FX_NUM_TIERS)(*([7] * _lib.FX_NUM_TIERS))
    st = lib.fx_batch_run_tiered(ref(a, "in", streams(a)), ref(a, "out", order(a)), a["flags"], None, counts)
    assert st == 0 or list(counts) == [7] * _lib.FX_NUM_TIERS  # a refused call leaves them alone
    return st


def pred_execute(lib, a):
    return lib.fx_pred_execute(ref(a, "in", pred(a)), ref(a, "out", order(a)), opt(a, "map"), a["lanes"], a["tier"],
                               opt(a, "state"), a["flags"], None)


def pred_run(lib, a):
    reruns = ctypes.c_uint32(7)  # written before the checks: a real word
    st = lib.fx_pred_run(ref(a, "in", pred(a)), ref(a, "out", order(a)), a["flags"], None, ctypes.byref(reruns))
    assert reruns.value == 0
    return st


def pending_aggregate(lib, a):
    return lib.fx_pending_aggregate(ref(a, "in", pending_in(a)), ref(a, "out", pending_out(a)), opt(a, "map"),
                                    a["lanes"], a["tier"], opt(a, "state"), None)


def pending_run(lib, a):
    reruns = ctypes.c_uint32(7)
    st = lib.fx_pending_run(ref(a, "in", pending_in(a)), ref(a, "out", pending_out(a)), None, ctypes.byref(reruns))
    assert reruns.value == 0
    return st


ENTRIES = {
    "execute": execute,
    "partial": partial,
    "run_tiered": run_tiered,
    "pred_execute": pred_execute,
    "pred_run": pred_run,
    "pending_aggregate": pending_aggregate,
    "pending_run": pending_run,
}
# what differs from VALID in an entry point's own valid set
OWN = {
    "partial": dict(flags=INIT | SAVE),
    "run_tiered": dict(flags=0),
    "pred_execute": dict(flags=0),
    "pred_run": dict(flags=0),
}

GRAPH_PLANES = ["in", "out", "dot", "hdr", "deps", "order", "release", "nexec", "err"]
PRED_PLANES = GRAPH_PLANES + ["clock_lo", "clock_hi"]
PENDING_PLANES = ["in", "out", "p_order", "p_nexec", "rifl", "count", "part", "head", "ready", "index", "nready",
                  "nopen", "p_err"]
GRAPH_SHAPE = [dict(n=0), dict(n=9), dict(dmax=32), dict(steps=1 << 26)]
PRED_SHAPE = [dict(n=0), dict(n=9), dict(dmax=PRED_MAX_DEPS + 1), dict(steps=1 << 26), dict(dmax=32, ndeps=False)]


def nulls(names):
    return [dict(null=name) for name in names]


# refused before the library looks for a device
MUTATIONS = {
    "execute": nulls(GRAPH_PLANES) + GRAPH_SHAPE,
    "partial": nulls(GRAPH_PLANES) + GRAPH_SHAPE,
    "run_tiered": nulls(GRAPH_PLANES) + GRAPH_SHAPE,
    "pred_execute": nulls(PRED_PLANES) + PRED_SHAPE,
    "pred_run": nulls(PRED_PLANES) + PRED_SHAPE,
    "pending_aggregate": nulls(PENDING_PLANES) + [dict(count_mask=0), dict(tier=2), dict(tier=2, state=True),
                                                  dict(tier=_lib.FX_PENDING_TIER_HBM), dict(state=True), dict(lanes=5)],
    "pending_run": nulls(PENDING_PLANES) + [dict(count_mask=0)],
}
# checked after the device, and refused before any launch
LATE = {
    "execute": [dict(end=9), dict(begin=5, end=4), dict(flags=0), dict(flags=INIT | SAVE), dict(lanes=5),
                dict(flags=INIT | PARTIAL), dict(tier=_lib.FX_NUM_TIERS), dict(tier=_lib.FX_NUM_TIERS, state=True),
                dict(tier=GLOBAL), dict(tier=WIDE_HBM), dict(tier=SPLIT), dict(tier=SPLIT, state=True, map=True),
                dict(tier=SPLIT, state=True, lanes=3), dict(tier=WIDE, end=4)],
    "partial": [dict(null="state"), dict(null="req"), dict(req_cap=0), dict(end=9), dict(begin=5, end=4),
                dict(flags=AT_COMMIT), dict(flags=INIT | PARTIAL)],
    "run_tiered": [dict(flags=_lib.first_tier_flag(_lib.FX_NUM_TIERS)), dict(flags=15 << _lib.FX_FLAG_TIER_SHIFT)],
    "pred_execute": [dict(lanes=5), dict(tier=3), dict(tier=3, state=True), dict(tier=_lib.FX_PRED_TIER_HBM),
                     dict(tier=_lib.FX_PRED_TIER_SMALL, state=True), dict(tier=_lib.FX_PRED_TIER_LDS, state=True)],
    "pred_run": [],
    "pending_aggregate": [dict(lanes=0x7FFFFFC1, map=True)],
    "pending_run": [],
}

# valid sets beside the entry point's own: every one reaches the device check
ALSO_VALID = {
    "execute": [dict(state=True), dict(flags=0, state=True), dict(flags=INIT | SAVE, state=True), dict(lanes=5, map=True),
                dict(lanes=0), dict(tier=GLOBAL, state=True), dict(tier=WIDE), dict(tier=WIDE_HBM, state=True),
                dict(tier=SPLIT, state=True), dict(dmax=31), dict(n=8), dict(dmax=0, null="deps"), dict(S=0, lanes=0),
                dict(begin=3, end=3)],
    "partial": [dict(flags=0), dict(flags=INIT), dict(S=0), dict(begin=8, end=8)],
    "run_tiered": [dict(flags=AT_COMMIT), dict(flags=_lib.first_tier_flag(WIDE_HBM)), dict(flags=INIT | SAVE), dict(S=0),
                   dict(dmax=31)],
    "pred_execute": [dict(flags=AT_COMMIT), dict(tier=_lib.FX_PRED_TIER_LDS), dict(tier=_lib.FX_PRED_TIER_HBM, state=True),
                     dict(lanes=5, map=True), dict(lanes=0), dict(dmax=PRED_MAX_DEPS), dict(dmax=31, ndeps=False),
                     dict(S=0, lanes=0)],
    "pred_run": [dict(flags=AT_COMMIT), dict(dmax=PRED_MAX_DEPS), dict(S=0), dict(n=8)],
    "pending_aggregate": [dict(tier=_lib.FX_PENDING_TIER_HBM, state=True), dict(lanes=5, map=True), dict(lanes=0),
                          dict(S=0, lanes=0), dict(steps=0)],
    "pending_run": [dict(S=0), dict(steps=0), dict(steps=1 << 26)],
}


def with_(entry, change):
    a = dict(VALID)
    a.update(OWN.get(entry, {}))
    a.update(change)
    return a


def rows(table):
    return [(entry, i) for entry in ENTRIES for i in range(len(table[entry]))]


def ids(table):
    return ["%s-%s" % (e, "-".join("%s_%s" % kv for kv in table[e][i].items())) for e, i in rows(table)]


@pytest.mark.parametrize("entry,i", rows(MUTATIONS), ids=ids(MUTATIONS))
def test_one_mutation_is_refused(lib, entry, i):
    assert ENTRIES[entry](lib, with_(entry, MUTATIONS[entry][i])) == _lib.FX_ERR_INVALID_ARG


@pytest.mark.parametrize("entry,i", rows(LATE), ids=ids(LATE))
def test_one_mutation_is_refused_after_the_device_check(lib, entry, i):
    want = _lib.FX_ERR_NO_DEVICE if lib.fx_device_count() <= 0 else _lib.FX_ERR_INVALID_ARG
    assert ENTRIES[entry](lib, with_(entry, LATE[entry][i])) == want


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_the_valid_sets_reach_the_device_check(lib, entry):
    """Without a device only: with one these calls would launch over the poison pointers."""
    if lib.fx_device_count() <= 0:
        for change in [{}] + ALSO_VALID[entry]:
            assert ENTRIES[entry](lib, with_(entry, change)) == _lib.FX_ERR_NO_DEVICE, change
