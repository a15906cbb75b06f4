"""The GC ring's restatement (tests/gc_ring_ref.py) against brute force, on the
CPU: seeded random histories of frontier moves for n in {3, 5, 7}, random link
delays, every GC interval of the GPU tests, and end times on and next to tick
times and delivery times, the stop on a delivery among them.  Whenever the
rings report nothing lost the two evaluations give the same Stable counts, and
the rings report a loss exactly when a look-up's entry was overwritten.  Then
the ring's edges by hand.  The kernel keeps no tick index any more: a tick's
report is the time query at the tick's own time, which is what the brute
force's enumerated deliveries check.
"""
import random

import pytest

import gc_ring_ref as R

GC_MS = [1, 3, 7, 10, 1000]


def random_case(rng, n, gc, depth):
    """(hist, d, end times with their stop pairs)"""
    d = [[0 if p == q else rng.randint(1, 120) for q in range(n)] for p in range(n)]
    span = rng.choice([150, 400]) if gc < 1000 else rng.choice([1500, 2500, 4000])
    hist = []
    for p in range(n):
        row = []
        for s in range(n):
            moves = rng.choice([0, 1, depth - 1, depth, depth + 1, 3 * depth, rng.randint(0, 4 * depth)])
            times = sorted(rng.choice([rng.randint(1, span), rng.randint(max(1, span - 150), span)])
                           for _ in range(moves))
            if moves > 2 and rng.random() < 0.5:
                times[1] = times[0]  # two moves in one millisecond
                times.sort()
            f, h = 0, []
            for t in times:
                f += rng.randint(1, 3)
                h.append((t, f))
            row.append(h)
        hist.append(row)
    ends = set()
    for _ in range(6):
        k = rng.randint(1, max(1, span // gc))
        p, q = rng.sample(range(n), 2)
        for base in (k * gc, k * gc + d[p][q]):
            for dt in (-1, 0, 1):
                if base + dt > 0:
                    ends.add((base + dt, None))
        ends.add((k * gc + d[p][q], (p, q)))  # the run stopped on this delivery
    ends.add((span + 1, None))
    return hist, d, sorted(ends, key=lambda e: (e[0], e[1] or (-1, -1)))


@pytest.mark.parametrize("n", [3, 5, 7])
@pytest.mark.parametrize("gc", GC_MS)
def test_ring_agrees_with_brute_force_or_reports_the_loss(n, gc):
    rng = random.Random(1000 * n + gc)
    seen = {True: 0, False: 0}
    for depth in (6, 12, 48):
        for _ in range(4):
            every, d, ends = random_case(rng, n, gc, depth)
            for tc, pair in ends:
                # a run that ends at tc has seen the moves up to tc
                hist = [[[m for m in h if m[0] <= tc] for h in row] for row in every]
                rings = [[R.ring_of(h, depth) for h in row] for row in hist]
                ok, got = R.finish_ring(n, rings, d, gc, tc, pair)
                lost, want = R.finish_brute(n, hist, d, gc, tc, pair, depth=depth)
                assert ok == (not lost), (n, gc, depth, tc, pair)
                if ok:
                    assert got == want, (n, gc, depth, tc, pair)
                seen[ok] += 1
    print("n %d gc %d: %d evaluations agree, %d report a loss" % (n, gc, seen[True], seen[False]))
    assert seen[True] > 0 and seen[False] > 0


def test_query_at_before_and_after_an_entry():
    r = R.ring_of([(10, 1), (20, 2), (30, 5)], 6)
    assert r.value_at(20) == (True, 2)  # exactly at an entry's time
    assert r.value_at(19) == (True, 1)  # one millisecond before it
    assert r.value_at(9) == (True, 0)   # before the first move: nothing moved yet
    assert r.value_at(10) == (True, 1)
    assert r.value_at(1000) == (True, 5)
    assert R.Ring(6).value_at(5) == (True, 0)  # no move at all


def test_two_moves_in_one_millisecond_the_newest_wins():
    r = R.ring_of([(10, 1), (20, 2), (20, 4), (30, 5)], 6)
    assert r.value_at(20) == (True, 4)
    assert r.value_at(29) == (True, 4)
    assert r.value_at(19) == (True, 1)


def test_ring_filled_exactly_and_by_one_more():
    full = [(10 * (i + 1), i + 1) for i in range(6)]
    r = R.ring_of(full, 6)
    assert r.count == 6 and None not in r.entries
    assert r.value_at(10) == (True, 1)
    assert r.value_at(9) == (True, 0)  # still known: nothing was overwritten
    assert not R.overwritten(full, 9, 6)
    more = full + [(70, 7)]
    r = R.ring_of(more, 6)
    assert r.value_at(70) == (True, 7)
    assert r.value_at(20) == (True, 2)  # the oldest entry left
    assert r.value_at(19) == (False, 0)  # answered by the overwritten move
    assert r.value_at(9) == (False, 0)   # "nothing moved yet" cannot be told from a loss
    assert R.overwritten(more, 19, 6) and R.overwritten(more, 9, 6) and not R.overwritten(more, 20, 6)
    # the ring wraps again and again: entry c mod depth
    many = [(i + 1, i + 1) for i in range(20)]
    r = R.ring_of(many, 6)
    assert sorted(e[1] for e in r.entries) == [15, 16, 17, 18, 19, 20]
    assert r.value_at(15) == (True, 15) and r.value_at(14) == (False, 0)


def test_tick_report_is_the_time_query_at_the_tick():
    """One source, two processes 5 ms apart, gc 10: tick 1 of process 0 fires
    at 20 and reports the frontier after every move up to 20, the move in its
    own millisecond included, and process 1 has it at 25."""
    h0 = [(5, 1), (20, 2), (21, 3)]
    h1 = [(8, 1), (24, 3)]
    hist = [[h0, []], [h1, []]]
    d = [[0, 5], [5, 0]]
    rings = [[R.ring_of(h, 6) for h in row] for row in hist]
    for tc, pair, want1 in [(25, None, 1), (26, None, 2), (25, (0, 1), 2), (15, None, 0), (16, None, 1)]:
        ok, got = R.finish_ring(2, rings, d, 10, tc, pair)
        lost, want = R.finish_brute(2, hist, d, 10, tc, pair, depth=6)
        assert ok and not lost and got == want and got[1] == want1, (tc, pair, got, want)


def test_depth_follows_the_launch_geometry():
    assert R.ring_depth(5, 5) == 6 and R.ring_depth(3, 3) == 6 and R.ring_depth(7, 7) == 6
    assert R.ring_depth(5, 10) == 12 and R.ring_depth(5, 20) == 24
    assert R.ring_depth(5, 5, wslots=256) == 48


def test_histories_from_commits_fill_gaps():
    adds = [[((1, 1), [], 10), ((1, 3), [], 12), ((2, 1), [], 12), ((1, 2), [], 15), ((1, 2), [], 16)], []]
    hist = R.histories_from_adds(2, adds)
    assert hist[0][0] == [(10, 1), (15, 3)] and hist[0][1] == [(12, 1)] and hist[1] == [[], []]
