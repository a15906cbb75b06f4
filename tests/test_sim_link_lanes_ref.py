"""tests/link_ring_ref.py on the CPU: the lane ring of the compiled-in
simulator builds (append with rank, pop with shift, overflow at D) against one
deque per link.

  batches   every target set of 1-4 targets of every sender (n = 5), into
            links that hold 0, D - 1 and D messages: the appended entries, the
            insertion seqs and the heads equal the one-by-one model's; a full
            target link fails the send and leaves every register as it was
  seqs      a batch's insertion seqs are consecutive in ascending target order
  shift     a link filled to D and drained: first in, first out, the head
            follows, and the emptied link's head is NONE without a count check
  random    seeded random sends and pops (the pop always the smallest (time,
            seq) head, as pop_min picks it), both models in step
  overflow  the same random traffic with an overflow list (a pool of 40): the
            lanes spill and refill, links run deeper than D, and the send
            fails exactly where the deques hold the pool's capacity"""
import itertools
import random

import pytest

import link_ring_ref as L

N = 5
DELAY = [[0 if p == q else 10 + 7 * p + 3 * q for q in range(N)] for p in range(N)]


def both(depth):
    return L.LaneRing(N, depth, DELAY), L.DequeLinks(N, depth, DELAY)


def same_state(ring, model):
    assert ring.seq == model.seq
    for l in range(ring.NP):
        assert ring.count[l] == len(model.q[l])
        assert ring.head(l) == model.head(l)
        got = [(ring.t[l][i], ring.s[l][i], (ring.kinds[l] >> (4 * i)) & 15, ring.w[l][i]) for i in range(ring.count[l])]
        assert got == list(model.q[l])
        # past the count: time and seq NONE (what a pop shifts into the head)
        assert all(ring.t[l][i] == L.NONE and ring.s[l][i] == L.NONE for i in range(ring.count[l], ring.D))


def fill(ring, model, p, q, count, now=0):
    for i in range(count):
        for x in (ring, model):
            x.append(now + i, p, 1 << q, 2, 1000 + i)


@pytest.mark.parametrize("depth", [2, 3, 4, 6])
@pytest.mark.parametrize("held", ["0", "D-1", "D"])
def test_batches_of_one_to_four_targets(depth, held):
    count = {"0": 0, "D-1": depth - 1, "D": depth}[held]
    for p in range(N):
        others = [q for q in range(N) if q != p]
        for k in range(1, 5):
            for targets in itertools.combinations(others, k):
                mask = sum(1 << q for q in targets)
                # the first target's link already holds `count` messages
                ring, model = both(depth)
                fill(ring, model, p, targets[0], count)
                same_state(ring, model)
                if count == depth:
                    before = (ring.t, ring.s, ring.w, ring.kinds, ring.count, ring.seq)
                    before = ([r[:] for r in before[0]], [r[:] for r in before[1]], [r[:] for r in before[2]],
                              before[3][:], before[4][:], before[5])
                    with pytest.raises(L.Capacity):
                        ring.append(100, p, mask, 3, 77)
                    with pytest.raises(L.Capacity):
                        model.append(100, p, mask, 3, 77)
                    assert (ring.t, ring.s, ring.w, ring.kinds, ring.count, ring.seq) == before
                else:
                    s0 = ring.seq
                    ring.append(100, p, mask, 3, 77)
                    model.append(100, p, mask, 3, 77)
                    same_state(ring, model)
                    # the one-by-one order: consecutive seqs, ascending targets
                    got = [ring.s[L.link_of(N, p, q)][ring.count[L.link_of(N, p, q)] - 1] for q in sorted(targets)]
                    assert got == list(range(s0, s0 + k))
                    assert ring.seq == s0 + k


@pytest.mark.parametrize("depth", [2, 4])
def test_fill_and_drain_is_first_in_first_out(depth):
    ring, model = both(depth)
    l = L.link_of(N, 3, 1)
    fill(ring, model, 3, 1, depth)
    for i in range(depth):
        assert ring.head(l) == (i + DELAY[3][1], i)
        assert ring.pop(l) == model.pop(l) == (i + DELAY[3][1], i, 2, 1000 + i)
        same_state(ring, model)
    assert ring.head(l) == (L.NONE, L.NONE) and ring.count[l] == 0
    # and it fills again from entry 0
    fill(ring, model, 3, 1, depth, now=50)
    same_state(ring, model)


@pytest.mark.parametrize("seed", range(4))
def test_random_sends_and_pops_stay_in_step(seed):
    rng = random.Random(seed)
    depth = 3
    ring, model = both(depth)
    now = 0
    failed = 0
    for _ in range(3000):
        if rng.random() < 0.45:
            p = rng.randrange(N)
            mask = rng.randrange(1, 1 << N) & ~(1 << p)
            kind, w2 = rng.randrange(5), rng.randrange(1 << 30)
            try:
                ring.append(now, p, mask, kind, w2)
                full = False
            except L.Capacity:
                full = True
            if full:
                failed += 1
                with pytest.raises(L.Capacity):
                    model.append(now, p, mask, kind, w2)
            else:
                model.append(now, p, mask, kind, w2)
        else:
            heads = [(ring.head(l), l) for l in range(ring.NP) if ring.count[l]]
            if heads:
                (t, _), l = min(heads)
                now = max(now, t)
                assert ring.pop(l) == model.pop(l)
        same_state(ring, model)
    assert failed > 0 and ring.seq > 1000


@pytest.mark.parametrize("seed", range(4))
def test_random_traffic_with_an_overflow_list(seed):
    rng = random.Random(100 + seed)
    depth, pool = 3, 40
    ring, model = L.LaneRing(N, depth, DELAY, pool), L.DequeLinks(N, depth, DELAY, pool)
    now = 0
    failed = deepest = 0
    for _ in range(4000):
        if rng.random() < 0.52:
            p = rng.randrange(N)
            mask = rng.randrange(1, 1 << N) & ~(1 << p)
            kind, w2 = rng.randrange(5), rng.randrange(1 << 30)
            try:
                ring.append(now, p, mask, kind, w2)
                full = False
            except L.Capacity:
                full = True
            if full:
                failed += 1
                assert sum(len(q) for q in model.q) + bin(mask).count("1") > pool
                with pytest.raises(L.Capacity):
                    model.append(now, p, mask, kind, w2)
            else:
                model.append(now, p, mask, kind, w2)
        else:
            heads = [(ring.head(l), l) for l in range(ring.NP) if ring.count[l]]
            if heads:
                (t, _), l = min(heads)
                now = max(now, t)
                assert ring.pop(l) == model.pop(l)
        assert ring.seq == model.seq and ring.nfree == pool - sum(len(q) for q in model.q)
        for l in range(ring.NP):
            assert ring.held(l) == len(model.q[l]) and ring.head(l) == model.head(l)
            assert (ring.kinds[l] >> 31 == 1) == (len(ring.lists[l]) > 0)
            assert not ring.lists[l] or ring.count[l] == depth
            deepest = max(deepest, ring.held(l))
    assert failed > 0 and deepest > depth + 2
