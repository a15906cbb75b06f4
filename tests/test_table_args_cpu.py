"""The argument checks of the table executor's entry points, one table over
fx_table_execute / _mk / _ps, fx_table_run / _mk / _ps, fx_table_advance,
fx_table_run_groups and fx_table_run_groups_capped: one valid argument set per
entry point, then one mutation per row, every one refused with
FX_ERR_INVALID_ARG before anything is dereferenced -- the pointers are poison
integers -- and before the library looks for a device.  The rows
tests/test_table_resume_cpu.py (fx_table_advance) and
tests/test_table_groups_cpu.py (fx_table_run_groups) already have are not
repeated.  CPU only."""
import ctypes

import pytest

from fantoch_amd import _lib

ONCHIP, HBM = _lib.FX_TABLE_TIER_ONCHIP, _lib.FX_TABLE_TIER_HBM
INIT, AT_COMMIT = _lib.FX_FLAG_INIT, _lib.FX_FLAG_EXECUTE_AT_COMMIT

NAMES = ("hdr", "dot", "clock", "votes", "nkeys", "order", "release", "nexec", "err", "stable", "sent", "map", "state",
         "route", "targets", "hsrc", "hdot", "hlen", "rounds")
POISON = {name: 0x5A5A0000 + 64 * i for i, name in enumerate(NAMES)}  # never dereferenced

# the valid set; S = 4 streams make two groups of two shards
VALID = dict(null=None, n=3, thr=2, vmax=1, keys=4, steps=8, S=4, flags=0, tier=ONCHIP, state=False, map=False,
             lanes=4, kind=_lib.FX_TABLE_KIND_PS, sent=True, shards=2, steps_out=12)


def ptr(a, name):
    return None if a["null"] == name else POISON[name]


def ref(a, name, obj):
    return None if a["null"] == name else ctypes.byref(obj)


def base(a):
    return _lib.TableBatch(ptr(a, "hdr"), ptr(a, "dot"), ptr(a, "clock"), ptr(a, "votes"), None, a["S"], a["steps"],
                           a["n"], a["keys"], a["vmax"], a["thr"])


def mk(a):
    return _lib.TableBatchMk(base(a), ptr(a, "nkeys"))


def order(a):
    return _lib.OrderBatch(ptr(a, "order"), ptr(a, "release"), ptr(a, "nexec"), ptr(a, "err"))


def execute(fn, batch, sent):
    def call(lib, a):
        args = (ref(a, "in", batch(a)), ref(a, "out", order(a)), POISON["stable"]) + ((POISON["sent"],) if sent else ())
        return getattr(lib, fn)(*args, POISON["map"] if a["map"] else None, a["lanes"], a["tier"],
                                POISON["state"] if a["state"] else None, a["flags"], None)
    return call


def run(fn, batch, sent):
    def call(lib, a):
        reruns = ctypes.c_uint32(7)  # written before the checks: a real word
        args = (ref(a, "in", batch(a)), ref(a, "out", order(a)), POISON["stable"]) + ((POISON["sent"],) if sent else ())
        return getattr(lib, fn)(*args, a["flags"], None, ctypes.byref(reruns))
    return call


def advance(lib, a):
    return lib.fx_table_advance(ref(a, "in", mk(a)), a["kind"], ref(a, "out", order(a)), POISON["stable"],
                                POISON["sent"] if a["sent"] else None, ptr(a, "state"), a["flags"], None)


def groups(capped):
    def call(lib, a):
        inb = _lib.TableGroupBatch(mk(a), ptr(a, "route"), ptr(a, "targets"), 16, a["shards"], a["steps_out"])
        outb = _lib.TableGroupOut(order(a), POISON["stable"], ptr(a, "sent"), ptr(a, "hsrc"), ptr(a, "hdot"),
                                  ptr(a, "hlen"), ptr(a, "rounds"))
        args = (ref(a, "in", inb), ref(a, "out", outb), ptr(a, "state"), a["flags"], None)
        return lib.fx_table_run_groups(*args) if capped is None else lib.fx_table_run_groups_capped(*args, capped)
    return call


ENTRIES = {
    "execute": execute("fx_table_execute", base, False),
    "execute_mk": execute("fx_table_execute_mk", mk, False),
    "execute_ps": execute("fx_table_execute_ps", mk, True),
    "run": run("fx_table_run", base, False),
    "run_mk": run("fx_table_run_mk", mk, False),
    "run_ps": run("fx_table_run_ps", mk, True),
    "advance": advance,
    "run_groups": groups(None),
    "run_groups_capped": groups(3),
}

PLANES = ["in", "out", "hdr", "dot", "clock", "votes", "order", "release", "nexec", "err"]
GROUP_PLANES = PLANES + ["nkeys", "state", "route", "targets", "sent", "hsrc", "hdot", "hlen", "rounds"]
SHAPE = [dict(n=0), dict(n=17), dict(thr=0), dict(thr=4), dict(vmax=0), dict(vmax=_lib.FX_TABLE_MAX_VOTES + 1),
         dict(keys=0), dict(keys=_lib.FX_TABLE_MAX_KEYS + 1), dict(steps=1 << 26)]
FLAGS = [dict(flags=4), dict(flags=1 << 8), dict(flags=INIT), dict(flags=INIT | AT_COMMIT)]
TIERS = [dict(tier=HBM), dict(tier=ONCHIP, state=True), dict(tier=2), dict(tier=2, state=True), dict(lanes=5)]
GROUP_SHAPE = [dict(steps=0), dict(shards=0), dict(shards=9), dict(shards=3), dict(steps_out=0),
               dict(steps_out=1 << 26)]


def nulls(names):
    return [dict(null=name) for name in names]


# what each entry point is asked beyond the rows the two older files hold
MUTATIONS = {
    "execute": nulls(PLANES) + SHAPE + FLAGS + TIERS,
    "execute_mk": nulls(PLANES + ["nkeys"]) + SHAPE + FLAGS + TIERS,
    "execute_ps": nulls(PLANES + ["nkeys"]) + SHAPE + FLAGS + TIERS,
    "run": nulls(PLANES) + SHAPE + FLAGS,
    "run_mk": nulls(PLANES + ["nkeys"]) + SHAPE + FLAGS,
    "run_ps": nulls(PLANES + ["nkeys"]) + SHAPE + FLAGS,
    # there: kind 3, the flags, every pointer, n 17, thr 0 and 4, steps 2^26, keys 0, stable_sent with another kind
    "advance": [dict(n=0), dict(vmax=0), dict(vmax=_lib.FX_TABLE_MAX_VOTES + 1),
                dict(keys=_lib.FX_TABLE_MAX_KEYS + 1)],
    # there: every pointer, the flags, shards, steps_out, steps, n 17, thr 0 and 4, keys 0
    "run_groups": [dict(n=0), dict(vmax=0), dict(vmax=_lib.FX_TABLE_MAX_VOTES + 1),
                   dict(keys=_lib.FX_TABLE_MAX_KEYS + 1), dict(flags=INIT | AT_COMMIT)],
    "run_groups_capped": nulls(GROUP_PLANES) + SHAPE + FLAGS + GROUP_SHAPE,
}
ROWS = [(entry, i) for entry in ENTRIES for i in range(len(MUTATIONS[entry]))]

# valid sets beside VALID itself: every one reaches the device check
ALSO_VALID = {
    "execute": [dict(flags=AT_COMMIT), dict(tier=HBM, state=True), dict(lanes=5, map=True), dict(lanes=0),
                dict(keys=_lib.FX_TABLE_ONCHIP_KEYS + 1), dict(vmax=_lib.FX_TABLE_MAX_VOTES), dict(n=16, thr=16),
                dict(keys=_lib.FX_TABLE_MAX_KEYS, tier=HBM, state=True), dict(S=0, lanes=0)],
    "execute_mk": [dict(flags=AT_COMMIT), dict(tier=HBM, state=True), dict(keys=_lib.FX_TABLE_ONCHIP_KEYS + 1)],
    "execute_ps": [dict(flags=AT_COMMIT), dict(tier=HBM, state=True), dict(keys=_lib.FX_TABLE_ONCHIP_KEYS + 1)],
    "run": [dict(flags=AT_COMMIT), dict(keys=_lib.FX_TABLE_ONCHIP_KEYS + 1), dict(S=0)],
    "run_mk": [dict(flags=AT_COMMIT), dict(keys=_lib.FX_TABLE_ONCHIP_KEYS + 1)],
    "run_ps": [dict(flags=AT_COMMIT), dict(keys=_lib.FX_TABLE_ONCHIP_KEYS + 1)],
    "advance": [dict(flags=INIT | AT_COMMIT), dict(S=0), dict(steps=0)],
    "run_groups": [dict(S=0)],
    "run_groups_capped": [dict(flags=AT_COMMIT), dict(S=0), dict(S=8, shards=8), dict(shards=1)],
}


def with_(change):
    a = dict(VALID)
    a.update(change)
    return a


@pytest.mark.parametrize("entry,i", ROWS, ids=["%s-%s" % (e, "-".join("%s_%s" % kv for kv in MUTATIONS[e][i].items()))
                                               for e, i in ROWS])
def test_one_mutation_is_refused(lib, entry, i):
    assert ENTRIES[entry](lib, with_(MUTATIONS[entry][i])) == _lib.FX_ERR_INVALID_ARG


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_the_valid_sets_reach_the_device_check(lib, entry):
    """Without a device only: with one these calls would launch over the poison pointers."""
    if lib.fx_device_count() <= 0:
        for change in [{}] + ALSO_VALID[entry]:
            assert ENTRIES[entry](lib, with_(change)) == _lib.FX_ERR_NO_DEVICE, change
