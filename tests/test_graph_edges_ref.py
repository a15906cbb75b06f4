"""The graph executor's restatement (graph_ref) and edge cases (graph_edges)
on the CPU: the unbounded restatement against the C++ oracle
(oracle/graph_oracle.cpp) on every stream of graph_edges and on generated
streams, its high-water marks against the oracle's, the condition every fit /
exceed pair must meet, and that the cases reach what their names say.

The oracle has no limits: it is compared with the unbounded restatement only.
What a tier's limits stop is argued from the restatement, whose counters name
the kernel lines they mirror (graph_ref's docstring)."""
import numpy as np
import pytest

import graph_edges as E
import graph_ref as R
from fantoch_amd import _lib
from fantoch_amd import streams as fs
from oracle import oracle_lib as O

CASES = E.all_cases() + E.hbm_cases()
RESUME = [E.resume_cuts(t) for t in (E.GROUP, E.LDS_LARGE, E.GLOBAL, E.LANE, E.WAVE, E.LANE_REG, E.WIDE_HBM)]


def same_as_oracle(planes, out, s, r):
    order, release, nexec, err, mp, mw = out
    k = int(nexec[s])
    o = [(int(x) & 0x7FFFFFFF, bool(int(x) & R.SCC_START)) for x in order[_lib.index(np.arange(k), s, planes.steps)]]
    rel = release[_lib.index(np.arange(planes.steps), s, planes.steps)]
    rel = {a: int(v) for a, v in enumerate(rel) if v != R.FX_RELEASE_NONE}
    assert (r["err"], r["nexec"]) == (int(err[s]), k), "stream %d" % s
    assert (r["order"], r["release"]) == (o, rel), "stream %d" % s
    assert r["pending"] == sorted(set(range(min(len(r["order"]) + len(r["pending"]), planes.steps))) - set(rel)) or \
        r["err"], "stream %d" % s
    assert (r["stats"]["max_pending"], r["stats"]["max_window"]) == (int(mp[s]), int(mw[s])), "stream %d" % s


@pytest.mark.parametrize("case", CASES + [c for c, _, _ in RESUME], ids=lambda c: c.name)
def test_unbounded_restatement_equals_oracle(case):
    for s in range(case.S):
        r = case.restated(s)
        assert r["err"] == 0 and r["row"] is None
        same_as_oracle(case.packed(), case.oracle(), s, r)


@pytest.mark.parametrize("kw", [dict(n=5, instances=20, cmds=60, window=8, cycle_pct=30),
                                dict(n=3, instances=30, cmds=50, window=6, cycle_pct=50),
                                dict(n=5, instances=8, cmds=100, window=24, cycle_pct=60),
                                dict(n=2, instances=33, cmds=40, window=5, cycle_pct=40),
                                dict(n=7, instances=8, cmds=40, window=12, cycle_pct=70, conflicts=(100,)),
                                dict(n=8, instances=4, cmds=30, window=0, cycle_pct=0)],
                         ids=lambda kw: "n=%d window=%d" % (kw["n"], kw["window"]))
def test_restatement_on_generated_streams(kw):
    planes = fs.synth_host(fs.synth_params(seed=11, **kw))
    out = O.batch_execute(planes, threads=8, stats=True)
    for s in range(planes.S):
        same_as_oracle(planes, out, s, R.run(planes.stream(s), planes.n))


PAIRS = [(c, p) for c in CASES for p in c.pairs]


@pytest.mark.parametrize("case,pair", PAIRS, ids=[c.name for c, _ in PAIRS])
def test_pair_condition(case, pair):
    """The fitting stream reaches the limit exactly and runs to its end; the named resource stops its twin at the
    expected row with the counter one over, nothing else would, and the two differ in one Add."""
    lim = R.tier_limits(pair.tier, case.n)
    fit, exc = case.restated(pair.fit, pair.tier), case.restated(pair.exceed, pair.tier)
    assert (fit["err"], fit["row"], fit["stop"]) == (0, None, None)
    assert case.fits(pair.fit, pair.tier) and not case.fits(pair.exceed, pair.tier)
    assert fit["stats"][pair.counter] == pair.limit
    assert fit == case.restated(pair.fit)  # the limits change nothing for a stream that fits
    assert (exc["err"], exc["stop"], exc["row"]) == (R.FX_ERR_CAPACITY, pair.resource, pair.row)
    assert exc["stats"][pair.counter] == pair.limit + 1
    unbounded = case.restated(pair.exceed)
    assert unbounded["err"] == 0 and R.exceeded(unbounded["stats"], lim) == [pair.resource]
    a, b = case.streams[pair.fit], case.streams[pair.exceed]
    rows = lambda st: [(x[0], tuple(x[1])) for x in st]
    if len(a) == len(b):
        assert sum(x != y for x, y in zip(rows(a), rows(b))) == 1
    else:
        i = next((i for i, (x, y) in enumerate(zip(rows(a), rows(b))) if x != y), len(a))
        assert len(b) == len(a) + 1 and rows(b)[:i] + rows(b)[i + 1:] == rows(a)
    # the limit is what the tier table reports
    assert pair.limit == {"slots": lim.P, "cache": lim.C, "window": lim.W - 1}[pair.resource]


def test_every_limit_of_every_tier_has_a_pair():
    have = set((p.tier, p.resource) for c in CASES for p in c.pairs)
    want = set((t, r) for t in E.LIMITED + (E.WIDE_HBM,) for r in ("slots", "window"))
    want |= set((t, "cache") for t in E.LIMITED if t not in (E.LANE_REG, E.WIDE))  # graph_edges' docstring
    assert have == want


def test_the_worklist_is_out_of_reach():
    """graph_edges' argument, on the largest cascades the slots hold: the high-water mark of a whole SCC of P is
    P, of the singletons waiting on one dot it is their number, both below every capacity; LANE_REG's masks stay
    lower still."""
    for tier in E.LIMITED:
        lim = R.tier_limits(tier, E.N)
        case = next(c for c in CASES if c.name == "worklist %s" % R.TIER_NAME[tier])
        ring, ring_waiter, star = (case.restated(s)["stats"] for s in range(3))
        assert (ring["wl"], ring["slots_all"]) == (lim.P, lim.P) and ring["wl"] <= lim.WLC
        assert ring_waiter["wl"] == lim.P - 1 and ring_waiter["wl_mask"] >= 1
        assert (star["wl"], star["slots_all"]) == (E.slots_held(lim), E.slots_held(lim) + 1)
        assert max(ring["wl_mask"], ring_waiter["wl_mask"], star["wl_mask"]) <= lim.P
    for case in CASES:
        for s in range(case.S):
            st = case.restated(s)["stats"]
            assert st["wl"] <= st["slots_all"] and st["wl_mask"] <= st["wl"]


def test_cases_reach_what_they_name():
    by = {c.name: c for c in CASES}
    hbm = R.tier_limits(E.WIDE_HBM, E.N)
    assert by["slots apart WIDE_HBM"].restated(0)["pending"] == list(range(hbm.P)) and hbm.P == 16384
    assert by["window WIDE_HBM"].restated(0)["stats"]["max_window"] == hbm.W == 32768
    for tier in E.LIMITED:
        name, lim = R.TIER_NAME[tier], R.tier_limits(tier, E.N)
        wide = by["widest %s" % name]
        assert wide.dmax == R.MAX_DEPS[tier] == max(len(a[1]) for a in wide.streams[0])
        assert wide.chain(tier)[0] == tier and all(wide.fits(s, tier) for s in range(wide.S))
        if lim.C is not None and tier != E.LANE_REG:  # more than C deps executed already, at most C kept
            assert R.MAX_DEPS[tier] - wide.restated(0)["stats"]["cache"] > lim.C >= wide.restated(0)["stats"]["cache"]
        assert wide.restated(1)["pending"]  # the second ends with the wide Add waiting
        win = by["window %s" % name]
        assert win.restated(0)["stats"]["max_window"] == lim.W  # highest exception, frontier 0
        assert win.restated(2)["pending"] and win.restated(0)["nexec"] == len(win.streams[0]) - 2
        assert win.restated(3)["nexec"] == len(win.streams[3]) - 1 and win.fits(3, tier)
        for S in (1, 63, 65, 130):
            pl = by["placement %s S=%d" % (name, S)]
            stopped = [s for s in range(S) if not pl.fits(s, tier)]
            assert stopped == sorted(set(s for s in E.PLACES + (S - 1,) if s < S))
            assert all(pl.fits(s, t) for s in range(S) if s not in stopped for t in E.LIMITED)
            if S > 1:
                assert set(len(st) for st in pl.streams) >= {0, 1}
    for tier in (E.LDS_LARGE, E.GLOBAL, E.WIDE):
        lim = R.tier_limits(tier, E.N)
        case = by["words %s" % R.TIER_NAME[tier]]
        highest = sorted(set(case.restated(s)["stats"]["off"] for s in range(case.S)))
        assert set(highest) >= {31, 32, 33, 63, 64, 65, lim.W - 2} and max(highest) == lim.W - 1  # with the gap
        assert all(case.fits(s, tier) for s in range(case.S))
    # the 1025th seq shares (1, 1)'s slot of the LDS wide tier's index: why that tier's frontier is stuck by a
    # late seq and not by a pending one
    held = R.run(E.stuck(1024, True, held=True), E.N, R.tier_limits(E.WIDE, E.N))
    assert (held["stop"], held["row"]) == ("index", 256)


def test_split_tiles_go_to_both_kernels():
    case = next(c for c in CASES if c.name == "split tiles")
    assert [case.tile_tier(s) for s in (0, 64, 128)] == [E.LANE_REG, E.GROUP, E.LANE_REG]
    stopped = [s for s in range(case.S) if not case.fits(s, E.SPLIT)]
    assert stopped == [5, 64 + 16, 129]
    assert not R.fits(case.restated(64 + 15)["stats"], E.LANE_REG, E.N) and case.fits(64 + 15, E.SPLIT)
    assert case.tier_counts(E.SPLIT)[:3] == [0, 3, 0] and case.tier_counts(E.SPLIT)[E.SPLIT] == case.S


def test_tier_counts_follow_the_chain():
    by = {c.name: c for c in CASES}
    slots = by["slots GROUP n=5"]  # 17 pending: GROUP stops it, LDS_LARGE holds it
    counts = slots.tier_counts(E.GROUP)
    assert (counts[E.GROUP], counts[E.LDS_LARGE], sum(counts)) == (2, 1, 3)
    cache = by["cache GLOBAL"]  # 17 deps: too wide for GROUP, starts at LDS_LARGE, whose 8 cached deps stop both
    counts = cache.tier_counts(E.GROUP)
    assert (counts[E.GROUP], counts[E.LDS_LARGE], counts[E.GLOBAL], counts[E.WIDE]) == (0, 2, 2, 1)
    wide = by["slots WIDE n=5"]
    assert wide.tier_counts(E.WIDE)[E.WIDE:] == [2, 1]


@pytest.mark.parametrize("case,cuts,marks", RESUME, ids=[c.name for c, _, _ in RESUME])
def test_resume_cuts_are_where_the_tables_are_full(case, cuts, marks):
    """At the slots row every vertex the tier has is taken (the wide tiers: but the one the next Add gets; all
    16384 at FX_TIER_WIDE_HBM, where nothing more arrives); at the window row the highest executed exception is
    window_bits above the frontier, every bit below it set."""
    tier = case.tiers[0]
    lim = R.tier_limits(tier, E.N)
    slots_row, window_row, held = marks
    assert all(case.fits(s, tier) for s in range(case.S))
    taken = R.run(case.streams[0][:slots_row], E.N)
    assert len(taken["pending"]) == slots_row == (lim.P if tier == E.WIDE_HBM else E.slots_held(lim))
    assert set((slots_row - 1, slots_row, slots_row + 1)) <= set(cuts)
    full = R.run(case.streams[1][:window_row], E.N)
    assert (full["stats"]["max_window"], len(full["pending"]), full["nexec"]) == (lim.W, held, lim.W - 1)
    assert set((32, 33, window_row)) <= set(cuts)
    if R.CACHE[tier]:
        assert R.run(case.streams[2][:1], E.N)["stats"]["cache"] == R.CACHE[tier]
