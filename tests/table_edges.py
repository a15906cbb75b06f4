"""Event streams that put the table executor's votes windows, pending-op
capacities and voter columns at their edges -- what the generated streams of
fantoch_amd.table.synth_table_streams* leave out: their clocks stay below a
few hundred, so the HBM ring of FX_TABLE_HBM_WINDOW bits never wraps, and the
ranges of one (key, voter) never overlap.  Plain Python, deterministic by
seed; tests/test_table_edges_ref.py holds what the restatement says of them,
tests/test_table_edges_gpu.py runs them on the GPU."""
import random

from table_ref import EventSet

FX_ERR_CAPACITY = 2
ONCHIP_WINDOW, HBM_WINDOW = 32, 2048  # FX_TABLE_ONCHIP_WINDOW, FX_TABLE_HBM_WINDOW


def walk(key, voter, frm, to, chunk):
    """Detached ranges that start at the frontier `frm` and move it to `to`,
    each at most `chunk` long (None: one range)."""
    out, f = [], frm
    while f < to:
        e = to if chunk is None else min(to, f + chunk)
        out.append(("D", key, [(voter, f + 1, e)]))
        f = e
    return out


def lift(stream, B, n, keys, chunk=None):
    """The stream with B added to every clock and vote, behind a prefix that
    walks every (key, voter) frontier from 0 to B.  StableAtShard events stay
    as they are.  Returns (events, length of the prefix)."""
    pre = [ev for k in range(keys) for v in range(1, n + 1) for ev in walk(k, v, 0, B, chunk)]
    out = []
    for ev in stream:
        if ev[0] == "A":
            out.append(ev[:3] + (ev[3] + B, [(v, s + B, e + B) for v, s, e in ev[4]]) + tuple(ev[5:]))
        elif ev[0] == "D":
            out.append(("D", ev[1], [(v, s + B, e + B) for v, s, e in ev[2]]))
        else:
            out.append(ev)
    return pre + out, len(pre)


def lifted_ref(ref, B, pre):
    """What the restatement must say of lift(stream, B, ...) given what it says
    of the stream: order and release rows move by the prefix, every stable
    clock by B (a key the stream never uses stands at B)."""
    out = dict(ref, order=[a + pre for a in ref["order"]],
               release={a + pre: r + pre for a, r in ref["release"].items()}, stable=[c + B for c in ref["stable"]])
    if "sent" in ref:
        out["sent"] = {a + pre: r + pre for a, r in ref["sent"].items()}
    return out


def highest(stream):
    """The highest clock or vote of a stream."""
    top = 0
    for ev in stream:
        if ev[0] == "A":
            top = max([top, ev[3]] + [e for _, _, e in ev[4]])
        elif ev[0] == "D":
            top = max([top] + [e for _, _, e in ev[2]])
    return top


def gappy(seed, n, keys, events, win):
    """Single-key commands over ranges that leave gaps and overlap: each event
    picks a key and a voter, an end within `win` of that voter's frontier
    (exactly `win` above it one time in 16) and a start up to 100 below the
    end; a range that adds no new vote is dropped.  Every fifth event is
    attached, its clock up to win // 2 above the frontier its range leaves,
    so ops pend and leave in groups."""
    rng = random.Random(seed)
    sets = {(k, v): EventSet() for k in range(keys) for v in range(1, n + 1)}
    seqs = [0] * (n + 1)
    out = []
    while len(out) < events:
        k, v = rng.randrange(keys), 1 + rng.randrange(n)
        es = sets[k, v].copy()
        end = es.frontier + (win if rng.randrange(16) == 0 else 1 + rng.randrange(win))
        start = max(1, end - rng.randrange(101))
        if not es.add_range(start, end):
            continue
        sets[k, v] = es
        if len(out) % 5 == 4:
            p = 1 + rng.randrange(n)
            seqs[p] += 1
            out.append(("A", k, (p, seqs[p]), es.frontier + 1 + rng.randrange(win // 2), [(v, start, end)]))
        else:
            out.append(("D", k, [(v, start, end)]))
    return out


def partly_seen(stream, n, keys):
    """(ranges that add a new vote and hold one seen before, ranges) of a
    stream of valid ranges, counted with an EventSet per (key, voter)."""
    sets = {(k, v): EventSet() for k in range(keys) for v in range(1, n + 1)}
    partly = total = 0
    for ev in stream:
        for v, s, e in (ev[4] if ev[0] == "A" else ev[2]):
            es = sets[ev[1], v]
            old = sum(1 for x in range(s, e + 1) if x <= es.frontier or x in es.above)
            assert es.add_range(s, e)
            partly += 0 < old
            total += 1
    return partly, total


def mass(P, n, seed=0):
    """P attached events on key 0 without votes -- clocks 1 + i % 7, dots
    (1 + i % n, 1 + i // n), shuffled -- then one detached (v, 1, 7) per
    voter: the event that makes clock 7 stable releases all P at once."""
    ops = [("A", 0, (1 + i % n, 1 + i // n), 1 + i % 7, []) for i in range(P)]
    random.Random(seed).shuffle(ops)
    return ops + [("D", 0, [(v, 1, 7)]) for v in range(1, n + 1)]


def window_edge(F, W, over, n=3):
    """Voter 1 of key 0 at frontier F; an op at clock F + 1; a vote exactly at
    the window's end (over = 0) or one beyond (over = 1); a range that fills
    the window but for F + 1 and crosses each of its words; then F + 1, so the
    frontier walks the whole window in one event; then the other voters.
    Returns (events, row of the gap vote)."""
    top = F + W + over
    st = walk(0, 1, 0, F, W) + [("A", 0, (1, 1), F + 1, [])]
    gap = len(st)
    st += [("D", 0, [(1, top, top)]), ("D", 0, [(1, F + 2, F + W - 1)]), ("D", 0, [(1, F + 1, F + 1)])]
    for v in range(2, n + 1):
        st += walk(0, v, 0, top, W)
    return st, gap


def seen_inside(F, W):
    """Three streams that end in a range wholly above the frontier F and
    wholly seen before (FX_ERR_VOTE_RANGE at the last event): the range again
    after a partly seen one, the range twice in one event, a part of it."""
    head = [("A", 0, (1, 1), 1, [(1, 1, 1), (2, 1, 1)])] + walk(0, 1, 1, F, W)
    r = (1, F + 5, F + 9)
    return [head + [("D", 0, [r]), ("D", 0, [(1, F + 7, F + 12)]), ("D", 0, [r])],
            head + [("D", 0, [r, r])],
            head + [("D", 0, [r]), ("D", 0, [(1, F + 6, F + 8)])]]


def max_votes_event(n=16, repeat=False):
    """One attached event with FX_TABLE_MAX_VOTES = 64 ranges, four disjoint
    ones per voter; with `repeat` the 64th repeats the 63rd."""
    votes = [(v, 1 + 4 * j, 2 + 4 * j) for v in range(1, n + 1) for j in range(4)]
    if repeat:
        votes[-1] = votes[-2]
    return [("A", 0, (1, 1), 2, votes)]


def stopped(run_stream, stream, at, n, thr, keys):
    """What a tier must leave of a stream that runs out of capacity at event
    `at`: the restatement of the events before it, with that status."""
    ref = run_stream(stream[:at], n, thr, keys)
    assert ref["err"] == 0
    return dict(ref, err=FX_ERR_CAPACITY)
