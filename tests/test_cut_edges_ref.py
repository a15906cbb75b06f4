"""The cut analysis restated (cut_ref) and its edge cases (cut_edges) on the
CPU: the restatement's cut flags against the flags the oracle's release plane
gives by itself, the driver's plan carried out by the oracle (renumbered
segments run alone and mapped back) against the oracle on the unsplit stream,
that every case reaches the limit it is named for, and that every case tells
a deliberately wrong restatement from the right one.

The expected figures of a case are worked out here from how it is laid down
(the segments a builder put, or by hand in a comment), not read from cut_ref."""
import numpy as np
import pytest

import cut_edges as E
import cut_ref as R
from fantoch_amd import _lib

CASES = E.all_cases()
BY = {c.name: c for c in CASES}


def laid(case, streams=None):
    """(segments, singles, longest, multi) of the streams laid down as whole segments."""
    segs = [k for s, l in enumerate(case.planes().laid) if streams is None or s in streams for k in l]
    return len(segs), segs.count(1), max(segs + [1]), len(segs) - segs.count(1)


def flags_equal_the_oracles(case):
    p, release = case.planes(), case.oracle()[1]
    checked = 0
    for st in case.analysis().streams:
        if st.bad:
            continue  # the oracle knows no dot range, stops at a double dot and keeps an index-only record pending
        got = R.oracle_flags(release, st.s, st.L, p.steps)
        assert np.array_equal(got, st.flags), "%s stream %d: flags differ at step %d" % (
            case.name, st.s, int(np.flatnonzero(got != st.flags)[0]))
        checked += 1
    return checked


def plan_equals_the_oracle(case, by_source=True):
    p = case.planes()
    order, release, nexec, err = case.oracle()
    for s, (o, r) in E.through_segments(case, by_source).items():
        rows = _lib.index(np.arange(len(o)), s, p.steps)
        assert (int(nexec[s]), int(err[s])) == (len(o), 0), "%s stream %d" % (case.name, s)
        assert np.array_equal(order[rows], o), "%s stream %d: order" % (case.name, s)
        assert np.array_equal(release[rows], r), "%s stream %d: release" % (case.name, s)


def test_constants_are_the_sources():
    """The limits the cases are built on, as graph_cut.hip has them today: a changed one fails here first."""
    assert (R.INF, R.MAX_SEG, R.CHUNK, R.BT, R.SMALL_S, R.NCLS) == (0xFFFFFFFF, 4096, 1024, 256, 64, 16)
    assert (R.RANK_INLINE, R.RANK_CLASS_MIN, R.BLK_ABOVE, R.TILE_STREAMS) == (4, 3, 64, 64)
    assert (R.SPARSE_ABOVE, R.RANK_SLOTS_FACTOR) == (1 << 32, 8)
    assert [R.seg_class(k) for k in (1, 2, 3, 4, 5, 8, 9, 4096, 4097)] == [0, 1, 2, 2, 3, 3, 4, 12, 13]


@pytest.mark.parametrize("case", [c for c in CASES if not c.at_commit], ids=lambda c: c.name)
def test_flags_equal_the_oracles(case):
    assert flags_equal_the_oracles(case) >= 1


@pytest.mark.parametrize("case", [c for c in CASES if not c.at_commit], ids=lambda c: c.name)
def test_the_plan_carried_out_by_the_oracle_equals_the_oracle(case):
    plan_equals_the_oracle(case)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_stopped_streams_stop_where_the_oracle_does(case):
    """A double dot stops the oracle itself at the row cut_edges names, with the outputs of the rows before."""
    from oracle import oracle_lib
    p = case.planes()
    full = oracle_lib.batch_execute(p, execute_at_commit=case.at_commit, threads=8)
    for s, (row, err) in case.stops().items():
        if err == _lib.FX_ERR_DOUBLE_INDEX:
            assert int(full[3][s]) == err and int(full[2][s]) == int(case.oracle()[2][s])
            rows = _lib.index(np.arange(row), s, p.steps)
            assert np.array_equal(full[1][rows], case.oracle()[1][rows])
    assert all(int(full[3][s]) == 0 for s in range(p.S) if s not in case.stops())


# ------------------------------------------------------------------ every case sits on its limit
def reached(case, nch, scan, rank, stats, classes, whole=None, slots=None):
    a = case.analysis()
    assert (a.nch, a.scan_kernel, a.rank_kernel) == (nch, scan, rank), case.name
    assert a.stats() == dict(zip(("segments", "single_segments", "max_segment", "whole_streams"), stats)), case.name
    assert set(c for c, k in enumerate(a.class_counts) if k and c) == set(classes), case.name
    assert {st.s: st.reasons for st in a.streams if st.whole} == (whole or {}), case.name
    if slots is not None:
        assert a.slots == slots, case.name
    assert not a.sparse


def test_block_edge_reaches_the_block_carry():
    case, e = BY["block edge"], R.CHUNK
    # segments: 1022 + 1023 + 1024 (a 2-cycle ends each), 2051 - 3, 2051 - 2, 2051 - 1025 (5 .. 1030),
    # 2051 - 1050 (1000 .. 2050); 8 of them longer than one Add
    reached(case, 3, "k_chunk_excl", "k_rank", (9193, 9185, 1051, 0), {1, 2, 11}, slots=8)
    st = case.analysis().streams
    assert [x.L for x in st[:3]] == [e - 1, e, e + 1] and all(x.segments[-1] == (x.L - 2, x.L - 1) for x in st[:3])
    assert (e - 2, e + 1) in st[3].segments  # a 4-cycle over the edge
    assert st[4].flags[e - 1] and (e, e + 1) in st[4].segments  # a cut exactly at the block's last step
    assert (5, e + 6) in st[5].segments and (e - 24, 2 * e + 2) in st[6].segments
    assert st[6].reach[e:2 * e].max() < 2 * e + 2  # block 1 adds nothing to the carry it passes on


def test_max_seg_reaches_both_sides():
    case, M = BY["MAX_SEG"], R.MAX_SEG
    # exact: 7 segments, 4 singles; every: 33 - 1 segments, 10 singles; over (whole): 11 segments, 5 of them
    # longer than one Add, which keep their batch slots: 3 + 22 + 5
    reached(case, 9, "k_chunk_excl", "k_rank", (39, 14, M, 1), set(range(1, 14)), {1: [R.OVER_MAX_SEG]}, slots=30)
    a = case.analysis()
    assert laid(case, (0, 2))[:3] == (39, 14, M) and laid(case, (1,))[:3] == (11, 6, M + 1)
    assert a.class_counts[12:14] == [2, 1] and a.streams[0].cls.max() == 12 and a.streams[1].cls.max() == 13
    assert sorted(a.streams[2].length[a.streams[2].length > 1].tolist()) == \
        sorted([1 << c for c in range(1, 12)] + [(1 << c) + 1 for c in range(1, 12)])
    assert a.streams[1].singles() > 0 and a.streams[1].start[int(np.argmax(a.streams[1].length))] > 0


@pytest.mark.parametrize("S,steps", [(1, 41), (63, 42), (64, 43), (65, 44), (130, 45)])
def test_streams_cases_reach_both_sides_of_the_switches(S, steps):
    case = BY["streams S=%d" % S]
    p, a = case.planes(), case.analysis()
    assert (p.S, p.steps, p.steps % 4) == (S, steps, {1: 1, 63: 2, 64: 3, 65: 0, 130: 1}[S])
    assert a.small == (S <= 64) and (S <= R.SMALL_S) == (S <= R.TILE_STREAMS)
    if S > 1:
        assert {0, 1, steps} <= set(p.lengths.tolist()) and len(set(p.lengths.tolist())) > 10
    segments, singles, longest, multi = laid(case)
    reached(case, 1, "k_chunk_excl", "k_rank", (segments, singles, longest, 0), {1, 2, 3}, slots=multi)
    assert S * steps > R.BT or S == 1  # more than one block of the flat kernels


def test_64_chunks_reach_both_scan_kernels():
    for steps, nch, scan, twos in ((65536, 64, "k_chunk_excl", 63), (65537, 65, "k_chunk_excl_blk", 64)):
        case = BY["64 chunks steps=%d" % steps]
        # across: a 2-cycle over each multiple of 1,024 below steps; into (one step shorter): segments of 31,
        # 2001, 21, 2770 and steps - 2 - 64000 + 1 Adds
        last = steps - 1 - 64000
        total = 2 * steps - 1 - twos - (30 + 2000 + 20 + 2769 + last - 1)
        reached(case, nch, scan, "k_rank_slots", (total, total - twos - 5, 2770, 0), {1, 5, 11, 12}, slots=twos + 5)
        a = case.analysis()
        assert all((k * R.CHUNK - 1, k * R.CHUNK) in set(a.streams[0].segments) for k in range(1, twos + 1))
        into = a.streams[1].segments
        assert all(seg in into for seg in ((1000, 1030), (3000, 5000), (10230, 10250), (30000, 32769)))
        assert [b // R.CHUNK - a0 // R.CHUNK for a0, b in into if b > a0] == [1, 2, 1, 3, 1]


def test_class_chunks_reach_the_chunk_edges():
    for NS, multi in ((1023, 68), (1024, 69), (1025, 70), (2049, 72)):
        case = BY["class chunks NS=%d" % NS]
        segments, singles, longest, m = laid(case)
        assert (segments, m) == (NS, multi)
        a = case.analysis()
        reached(case, a.nch, "k_chunk_excl", "k_rank", (NS, NS - multi, 65, 0), range(1, 8), slots=multi)
        assert (a.NS, a.class_chunks) == (NS, (NS + 1023) // 1024)
        cls = np.concatenate([st.cls for st in a.streams])  # by segment id
        assert len(a.streams[0].end) == 70  # the second stream's ids start past a wave's edge
        for i in (63, 64, 255, 256, 1023, 1024, 2047, 2048):
            assert i >= NS or cls[i] > 0
        assert cls[320:384].tolist() == [1 + i % 7 for i in range(64)]  # one wave's ballots, every class in it


def test_rank_path_reaches_both_kernels():
    for steps, rank in ((512, "k_rank"), (513, "k_rank_slots")):
        case = BY["rank path steps=%d" % steps]
        segments, singles, longest, multi = laid(case)
        reached(case, 1, "k_chunk_excl", rank, (segments, singles, 17, 0), {2, 3, 4, 5}, slots=5)
        a = case.analysis()
        # 5, 8 -> class 3 (8 each), 9 -> 4 (16), 17 -> 5 (32): 64 Adds at most, and 64 * 8 = 512
        assert (a.nl, a.nl_adds, case.planes().S * steps) == (4, 64, steps)
        assert sorted(k for k in case.planes().laid[0] if k > 1) == sorted(E.RANKED)
        assert min(E.RANKED) == R.RANK_INLINE and R.RANK_INLINE + 1 in E.RANKED  # either side of RANK_INLINE


def test_dots_cases_reach_what_they_name():
    case = BY["dots n=8"]
    # sparse 6 segments (4 singles), wide 27 (26), own 4 (3), plain 3 (2) twice; the four with a dep that never
    # arrives run whole, their 2-cycles keep batch slots: 2 + 1 + 1 + 2 + 4 * 2
    reached(case, 1, "k_chunk_excl", "k_rank_slots", (43, 37, 7, 4), {1, 2, 3},
            {s: [R.NO_FINAL_CUT] for s in (1, 3, 5, 7)}, slots=12 - 2)
    p, a = case.planes(), case.analysis()
    assert (p.n, p.dmax) == (8, 31) and case.first_tier() == 1
    sparse, wide, own = a.streams[0], a.streams[2], a.streams[4]
    assert sorted(sparse.length.tolist()) == [1, 1, 1, 1, 3, 5] and sparse.max_seq == 1000000
    assert 3 <= R.RANK_INLINE < 5  # the 3-cycle is ranked by k_build, the 5-cycle by k_rank / k_rank_slots
    k = int(np.argmax(wide.length))
    assert int(wide.nd.max()) == 31 and len(wide.renumber(k)[0][1]) == 6 and wide.length[k] == 7
    assert own.reach.tolist() == [0, 1, 3, 3, 4] and own.renumber(2)[0][1] == [(3, 1), (4, 1)]  # its own dot stays
    for s, dep in ((1, (0, 1)), (3, (9, 1)), (5, (1, 8)), (7, (2, 7))):
        st = a.streams[s]
        row = int(np.flatnonzero(st.reach == R.INF)[0])
        assert _lib.unpack_dot(st.deps[0][row]) == dep and st.flags[row - 1] and not st.flags[row:].any()
        assert 0 < st.singles() < len(st.end)  # singles and a 2-cycle before it
        assert st.max_seq == 7 and (st.dot == E.pk(1, 7)).any() and not (st.dot == E.pk(2, 7)).any()
    reached(BY["dots n=1"], 1, "k_chunk_excl", "k_rank", laid(BY["dots n=1"])[:3] + (0,), {1, 2, 3, 4, 5}, slots=5)
    reached(BY["dots dmax=0"], 1, "k_chunk_excl", "k_rank_slots", (15, 15, 1, 0), (), slots=0)
    assert BY["dots dmax=0"].planes().dmax == 0 and BY["dots n=1"].planes().n == 1


def test_whole_beside_cut_has_every_reason():
    case = BY["whole beside cut"]
    segments, singles, longest, multi = laid(case, (0, 2, 4, 6, 8, 10))
    whole = {1: [R.BAD_SOURCE], 3: [R.DOUBLE_DOT, R.NO_FINAL_CUT], 5: [R.NOT_AN_ADD], 7: [R.NO_FINAL_CUT],
             9: [R.OVER_MAX_SEG]}
    reached(case, 5, "k_chunk_excl", "k_rank_slots", (segments, singles, longest, 5), {1, 2, 3, 13}, whole)
    a = case.analysis()
    assert a.racy and case.stops() == {1: (9, _lib.FX_ERR_DOT_RANGE), 3: (11, _lib.FX_ERR_DOUBLE_INDEX)}
    for s in whole:  # singles and longer segments before the step that spoils it
        st = a.streams[s]
        assert st.length[:6].tolist() == E.BEFORE and st.singles() >= 4
    assert sum(a.streams[s].singles() for s in whole) > 0 and a.NS - a.slots > a.single_segments


def test_sparse_fallback_and_execute_at_commit():
    a = BY["sparse fallback"].analysis()
    assert a.sparse and a.ptotal == 33 * 8 * (1 << 24) > R.SPARSE_ABOVE and 32 * 8 * (1 << 24) <= R.SPARSE_ABOVE
    case = BY["execute at commit"]
    order, release, nexec, err = case.oracle()
    p = case.planes()
    assert nexec.tolist() == p.lengths.tolist() and laid(case)[3] > 0
    for s in range(p.S):
        rows = _lib.index(np.arange(int(nexec[s])), s, p.steps)
        assert np.array_equal(release[rows], np.arange(len(rows)))


# ------------------------------------------------------------------ every case tells a wrong restatement
def differs(case, **variant):
    """What a wrong restatement changes on the case: the flags, the stats."""
    right, wrong = case.analysis(), R.analyse(case.planes(), **variant)
    flags = any(not np.array_equal(x.flags, y.flags) for x, y in zip(right.streams, wrong.streams))
    return flags, right.stats() != wrong.stats()


def test_no_carry_across_blocks_is_caught():
    for name in ("block edge", "64 chunks steps=65536", "64 chunks steps=65537"):
        assert differs(BY[name], no_carry=R.CHUNK) == (True, True), name
    wrong = R.analyse(BY["block edge"].planes(), no_carry=R.CHUNK)
    e = R.CHUNK
    assert wrong.streams[5].flags[e:e + 6].all() and wrong.streams[6].flags[e:2 * e].all()  # both carries
    assert wrong.streams[6].flags[2 * e:2 * e + 2].all()  # .. and the one through the block that adds nothing
    # (the cycles over the edge do not tell: each of their Adds names the next, so the block's own maximum holds)
    assert differs(BY["64 chunks steps=65537"], no_carry=R.CHUNK * R.CHUNK) == (False, False)  # one round only


def test_max_seg_off_by_one_is_caught():
    M = R.MAX_SEG
    assert R.analyse(BY["MAX_SEG"].planes(), max_seg=M - 1).whole == [0, 1]
    assert R.analyse(BY["MAX_SEG"].planes(), max_seg=M + 1).whole == []
    assert R.analyse(BY["MAX_SEG"].planes(), max_seg=M + 1).max_segment == M + 1
    assert R.analyse(BY["whole beside cut"].planes(), max_seg=M + 1).whole == [1, 3, 5, 7]
    for name in ("MAX_SEG", "whole beside cut"):
        assert differs(BY[name], max_seg=M + 1) == (False, True)


def test_singles_counted_over_all_streams_are_caught():
    """What the driver reported before (NS - h_nbatch): on both cases more than the cut streams' singles, on
    `whole beside cut` a figure the race of the double dot could move."""
    for name, before in (("MAX_SEG", 20), ("whole beside cut", None)):
        case = BY[name]
        wrong = R.analyse(case.planes(), singles="all")
        assert wrong.single_segments > case.analysis().single_segments
        assert wrong.single_segments == case.analysis().single_segments + sum(
            case.analysis().streams[s].singles() for s in case.analysis().whole)
        assert before is None or wrong.single_segments == before
        assert case.analysis().single_segments <= case.analysis().segments
    for case in CASES:  # and nowhere else does it matter: the other cases' whole streams have no single
        if case.name not in ("MAX_SEG", "whole beside cut", "dots n=8", "sparse fallback"):
            assert differs(case, singles="all") == (False, False), case.name


def test_a_rank_that_ignores_the_source_is_caught():
    case = BY["dots n=8"]
    sparse = case.analysis().streams[0]
    ring = int(np.flatnonzero(sparse.length == 5)[0])
    right, wrong = sparse.renumber(ring), sparse.renumber(ring, by_source=False)
    # (2, 5) (3, 7) (2, 900000) (3, 1) (2, 17): ranks per source 1 2 3 1 2, over all dots 2 3 5 1 4
    assert [d for d, _, _ in right] == [(2, 1), (3, 2), (2, 3), (3, 1), (2, 2)]
    assert [d for d, _, _ in wrong] == [(2, 2), (3, 3), (2, 5), (3, 1), (2, 4)]
    assert [deps for _, deps, _ in right] == [[(3, 2)], [(2, 3)], [(3, 1)], [(2, 2)], [(2, 1)]]
    inline = int(np.flatnonzero(sparse.length == 3)[0])
    assert [d for d, _, _ in sparse.renumber(inline)] == [(5, 1), (5, 3), (5, 2)]  # the order of sparse seqs kept
    # dense per-source ranks keep the segment's executed clock compact: the wrong ranks leave a source's
    # frontier stuck below dots that executed, which the right ones never do
    assert max(q for (s, q), _, _ in right) == 3 and max(q for (s, q), _, _ in wrong) == 5


# ------------------------------------------------------------------ the rounds case: built once, dropped after
def test_rounds_case():
    case = E.rounds_case()
    r = R.CHUNK * R.CHUNK
    assert case.planes().steps == r + R.CHUNK + 1
    assert flags_equal_the_oracles(case) == 1
    # one segment of 11 Adds (r - 6 .. r + 4, the 4-cycle inside it) and two 2-cycles: steps - 10 - 2 segments
    steps = case.planes().steps
    reached(case, 1026, "k_chunk_excl_blk", "k_rank_slots", (steps - 12, steps - 15, 11, 0), {1, 4}, slots=3)
    a = case.analysis()
    assert a.nch > R.CHUNK and a.class_chunks > R.CHUNK  # a second round in the max scan and in the sum scans
    st = a.streams[0]
    assert (r - 6, r + 4) in st.segments and st.reach[r - 2:r + 2].tolist() == [r - 1, r, r + 1, r + 1]
    late = len(st.end) - 1
    assert st.length[late] == 2 and late > r and st.length[10] == 2  # a batch slot either side of the rounds' edge
    wrong = R.analyse(case.planes(), no_carry=r)
    # without the first round's carry, r - 6's reach of r + 4 is lost: the 4-cycle ends its own segment at r + 1
    assert wrong.streams[0].flags[r:r + 4].tolist() == [False, True, True, True] and not st.flags[r:r + 4].any()
    assert wrong.stats() != a.stats()
    assert R.analyse(case.planes(), no_carry=R.CHUNK).stats() != a.stats()
    plan_equals_the_oracle(case)
