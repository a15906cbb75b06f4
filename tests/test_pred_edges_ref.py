"""The predecessors executor's restatement (pred_ref) and edge cases
(pred_edges) on the CPU: the unbounded restatement against the C++ oracle
(oracle/pred_oracle.cpp) on every shape and on the reference's own fixtures,
the condition every fit / exceed pair must meet, and the clock cases against
orders written out by hand.

Where the restatement and the oracle differ, by definition:
  * FX_ERR_DOT_RANGE (a committed dot with source 0, source above n or seq 0):
    the oracle has no such check and goes on, so from the failing row on only
    the restatement stops; what both executed before that row is compared.
Nothing else differs: FX_ERR_DOUBLE_INDEX is the oracle's too, and the oracle
has no limits (it is compared with limits=None only)."""
import itertools

import numpy as np
import pytest

import pred_edges as E
import pred_ref as R
import pred_shapes as PS
from fantoch_amd import _lib
from oracle import oracle_lib as O

CASES = E.all_cases()


def oracle_rows(planes, out, s):
    order, release, nexec, err = out
    k = int(nexec[s])
    o = [int(x) & 0x7FFFFFFF for x in order[_lib.index(np.arange(k), s, planes.steps)]]
    rel = release[_lib.index(np.arange(planes.steps), s, planes.steps)]
    return o, {a: int(v) for a, v in enumerate(rel) if v != R.FX_RELEASE_NONE}, int(err[s])


def same_as_oracle(streams, n, packed, at_commit=False, header_nd=False):
    planes, clo, chi, nd = packed
    out = O.pred_batch_execute(planes, clo, chi, threads=4, ndeps=None if header_nd else nd,
                               execute_at_commit=at_commit)
    for s, st in enumerate(streams):
        r = R.run(st, n, None, at_commit)
        o, rel, err = oracle_rows(planes, out, s)
        assert r["stop"] is None
        if r["err"] == R.FX_ERR_DOT_RANGE:  # the oracle does not stop: the rows before the failing one
            stop = min(len(st), planes.steps)
            bad = next(i for i, a in enumerate(st) if not (1 <= a[0][0] <= n and a[0][1] != 0))
            assert err in (0, R.FX_ERR_DOUBLE_INDEX)
            o = [a for a in o if rel[a] < bad]
            rel = {a: v for a, v in rel.items() if v < bad}
            assert stop >= bad
        else:
            assert err == r["err"], "stream %d" % s
        assert (o, rel) == (r["order"], r["release"]), "stream %d" % s


@pytest.mark.parametrize("at_commit", [False, True])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_unbounded_restatement_equals_oracle(case, at_commit):
    same_as_oracle(case.streams, case.n, case.packed(), at_commit, case.header_nd)


def test_restatement_on_the_reference_fixtures():
    """mod.rs:419-459 `simple`, and mod.rs:461-591 under every permutation."""
    r = R.run(PS.SIMPLE, 2)
    assert (r["order"], r["release"], r["err"]) == (PS.SIMPLE_ORDER, {0: 1, 1: 1}, 0)
    streams = []
    for args in PS.random_cases():
        for perm in itertools.permutations(range(len(args))):
            streams.append([(args[i][0], args[i][1], t, (args[i][2], 1)) for t, i in enumerate(perm)])
    same_as_oracle(streams, 2, PS.pack_pred_streams(streams, 2))
    assert all(R.run(st, 2)["nexec"] == len(st) for st in streams)


@pytest.mark.parametrize("n,events,keys,window", [(3, 40, 8, 0), (5, 30, 16, 12), (2, 80, 4, 0), (4, 16, 32, 4)])
def test_restatement_on_random_streams(n, events, keys, window):
    streams = PS.random_streams(7, 24, n, events, keys=keys, window=window)
    same_as_oracle(streams, n, PS.pack_pred_streams(streams, n))
    same_as_oracle(streams, n, PS.pack_pred_streams(streams, n), at_commit=True)


PAIRS = [(c, p) for c in CASES for p in c.pairs]
FIELD = dict(vertices="P", index="Q", window="W", frames="FD", lists="LL")


@pytest.mark.parametrize("case,pair", PAIRS, ids=[c.name for c, _ in PAIRS])
def test_pair_condition(case, pair):
    """The named resource stops the exceeding stream at its last row, the fitting stream peaks at the limit
    (less `short`) and finishes, and no other resource stops either."""
    lim = case.limits(pair.tier)
    fit, exc = case.restated(pair.fit, pair.tier), case.restated(pair.exceed, pair.tier)
    assert (fit["err"], fit["stop"]) == (0, None)
    assert fit["peak"][pair.resource] == getattr(lim, FIELD[pair.resource]) - pair.short
    assert (exc["err"], exc["stop"], exc["clock"]) == (R.FX_ERR_CAPACITY, pair.resource, pair.clock)
    assert exc["peak"][pair.resource] > getattr(lim, FIELD[pair.resource])
    # the stop is the exceeding stream's last row, or (the shifted ring walk) its first
    unbounded = case.restated(pair.exceed, None)
    assert unbounded["err"] == 0
    assert exc["row"] == (0 if case.name.startswith("window") else len(case.streams[pair.exceed]) - 1)
    # with that one resource unbounded nothing else stops it
    wide = lim._replace(**{FIELD[pair.resource]: 1 << 30})
    assert R.run(case.streams[pair.exceed], case.n, wide)["err"] == 0
    # the two streams differ by one command, or (the ring walks) by one seq
    a, b = case.streams[pair.fit], case.streams[pair.exceed]
    assert len(b) - len(a) in (0, 1)
    if len(a) == len(b):
        assert all(x[0][1] + 1 == y[0][1] for x, y in zip(a, b)) or \
            sum(x[0] != y[0] for x, y in zip(a, b)) == 1


def test_frames_are_reachable_in_the_compiled_layout_only():
    for tier, n, dmax in ((R.SMALL, 2, 1), (R.SMALL, 5, 4), (R.LDS, 2, 1), (R.LDS, 5, 5), (R.HBM, 2, 1)):
        lim = R.tier_limits(tier, n, dmax)
        assert lim.FD == lim.P
    assert R.tier_limits(R.SMALL, 5, 5).FD < R.tier_limits(R.SMALL, 5, 5).P
    assert R.tier_limits(R.SMALL, 5, 0) == R.tier_limits(R.SMALL, 5, 1) != R.tier_limits(R.SMALL, 5, 5)


def test_index_divides_window_in_every_layout():
    """Why no stream reaches seq - frontier - 1 == W on the executed clock (pred_edges' docstring)."""
    for tier, n, dmax in itertools.product((R.SMALL, R.LDS, R.HBM), (1, 2, 5, 8), (0, 1, 5, 31, 256)):
        lim = R.tier_limits(tier, n, dmax)
        assert lim is None or (lim.W % lim.Q == 0 and lim.Q & (lim.Q - 1) == 0)


def test_clock_cases_agree_with_the_hand_written_orders():
    for case in (c for c in CASES if c.hand):
        assert len(case.hand) == case.S == 2 * len(E.CLOCK_PAIRS)
        for s in range(case.S):
            for tier in (None,) + case.tiers:
                r = case.restated(s, tier)
                assert (r["order"], r["nexec"], r["err"]) == (case.hand[s], 2, 0), "stream %d" % s
                assert r["release"] == {0: 1, 1: 1}


def test_cases_reach_what_they_name():
    by = {c.name: c for c in CASES}
    dc = by["deps count"]
    assert dc.dmax == 256 and [len(st[-3][1]) if len(st) > 1 else 0 for st in dc.streams].count(256) == 6
    assert all(dc.restated(s, None)["nexec"] == len(dc.streams[s]) for s in range(dc.S))
    assert by["deps header"].dmax == 31
    for name in ("vertices compiled", "window compiled", "frames compiled", "lengths compiled", "lanes compiled 41"):
        assert (by[name].n, by[name].dmax) == (5, 5)  # what selects k_pred<false, 5, 5, WPB>
    planes = by["lengths"].packed()[0]
    assert sorted(set(len(st) for st in by["lengths"].streams)) == list(E.LENGTHS)
    assert planes.lengths.max() > planes.steps
    errs = [by["errors"].restated(s, None)["err"] for s in range(by["errors"].S)]
    assert errs == [R.FX_ERR_DOT_RANGE] * 7 + [R.FX_ERR_DOUBLE_INDEX] * 4
    assert [by["errors"].restated(s, None)["nexec"] for s in range(11)] == [0, 0, 0, 2, 2, 2, 0, 0, 0, 2, 2]
    assert [by["errors"].restated(s, None)["row"] for s in range(11)] == [0, 0, 0, 2, 2, 2, 1, 1, 2, 2, 2]
    # the executed frontier lags the committed one, and a phase is decided by ring bits
    st = by["stuck frontier SMALL"]
    r = st.restated(0, R.SMALL)
    assert r["pending"] == 3 and r["nexec"] == len(st.streams[0]) - 3
    # the ladder meets FX_ERR_CAPACITY at HBM too
    assert by["vertices HBM"].expected_ladder()[1:] == (4, R.FX_ERR_CAPACITY)
