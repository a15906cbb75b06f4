"""The restatement of the metrics pass (metrics_ref) and the edge cases built on it (metrics_edges), before
either side of the library is asked anything: known answers written out by hand, the CPU oracle's executor
outputs through the arithmetic the GPU parity tests used before they moved onto the restatement, and that every
case sits on the edge it is named after.  CPU only."""
import numpy as np
import pytest

import metrics_edges as E
import metrics_ref
from fantoch_amd import _lib
from fantoch_amd import streams as fs
from oracle import oracle_lib

FLAG = _lib.FX_ORDER_SCC_START
NONE = _lib.FX_RELEASE_NONE


def planes(S, steps, streams):
    """Planes over 0xA5 from {s: (times by arrival, order words, release by arrival, nexec)}."""
    pw = _lib.plane_words(S, steps)
    hdr, order, release = (np.full(pw, E.A5, np.uint32) for _ in range(3))
    nexec = np.full(S, E.A5, np.uint32)
    for s, (times, words, rel, ne) in streams.items():
        hdr[_lib.index(np.arange(len(times)), s, steps)] = times
        order[_lib.index(np.arange(len(words)), s, steps)] = words
        release[_lib.index(np.arange(len(rel)), s, steps)] = rel
        nexec[s] = ne
    return hdr, order, release, nexec


def hist(nbins, counts):
    h = np.zeros(nbins, np.uint64)
    for b, n in counts.items():
        h[b] = n
    return h


# ------------------------------------------------------------------ known answers
def test_known_answer_two_sccs_and_a_clamp():
    """Arrivals at 10, 12, 15, 30 ms; 0 runs at step 1, 1 and 2 (one SCC of two) at step 2, 3 at its own step.
    Delays 2, 3, 0, 0; SCCs of 1, 2 and 1 rows.  With 3 delay bins, 2 and 3 share the last one."""
    hdr, order, release, nexec = planes(1, 4, {0: ([10, 12, 15, 30], [0 | FLAG, 2 | FLAG, 1, 3 | FLAG], [1, 2, 2, 3], 4)})
    chain, delay = metrics_ref.hists(hdr, order, release, nexec, 1, 4, 4, 8)
    assert np.array_equal(chain, hist(4, {1: 2, 2: 1})) and np.array_equal(delay, hist(8, {0: 2, 2: 1, 3: 1}))
    chain, delay = metrics_ref.hists(hdr, order, release, nexec, 1, 4, 2, 3)
    assert np.array_equal(chain, hist(2, {1: 3})) and np.array_equal(delay, hist(3, {0: 2, 2: 2}))


def test_known_answer_rows_that_do_not_count():
    """Stream 0 of 5 rows, nexec 4: row 0 unflagged before any flag (delay 1, no SCC); row 1 flagged, its release
    NONE (no delay, and the SCC of rows 1 and 2 is skipped); row 2 unflagged, delay 4; row 3 flagged with rec ==
    steps (nothing); row 4 is above nexec.  Stream 1 has nexec = steps + 1 and gives nothing; stream 2 nexec 0."""
    top = 0xFF000000  # header bits 24..31 must not matter
    s0 = ([100 | top, 101 | top, 50 | top, 54 | top, 7], [0, 1 | FLAG, 2, 5 | FLAG, 3 | FLAG], [1, NONE, 3, 3, 4], 4)
    s1 = ([1, 2, 3, 4, 5], [k | FLAG for k in range(5)], [0, 1, 2, 3, 4], 6)
    hdr, order, release, nexec = planes(3, 5, {0: s0, 1: s1, 2: ([], [], [], 0)})
    chain, delay = metrics_ref.hists(hdr, order, release, nexec, 3, 5, 8, 8)
    assert np.array_equal(chain, hist(8, {})) and np.array_equal(delay, hist(8, {1: 1, 4: 1}))
    # the same with stream 1's count repaired: five SCCs of one row, five delays of 0
    nexec[1] = 5
    chain, delay = metrics_ref.hists(hdr, order, release, nexec, 3, 5, 8, 8)
    assert np.array_equal(chain, hist(8, {1: 5})) and np.array_equal(delay, hist(8, {0: 5, 1: 1, 4: 1}))


def test_known_answer_wrap_and_the_widest_delay():
    """A release earlier than the arrival: 5 - 9 as a u32 is 2^32 - 4, the last bin; 0xFFFFFF - 0 is the widest
    delay two headers can hold.  An SCC that nexec cuts."""
    s0 = ([9, 5, 0, 0xFFFFFF], [0 | FLAG, 2 | FLAG, 1, 3], [1, 1, 3, 3], 3)
    hdr, order, release, nexec = planes(1, 4, {0: s0})
    delays, sizes = metrics_ref.samples(hdr, order, release, nexec, 1, 4)
    assert sorted(delays) == [0, 0xFFFFFF, (1 << 32) - 4] and sorted(sizes) == [1, 2]
    chain, delay = metrics_ref.hists(hdr, order, release, nexec, 1, 4, 2, 5)
    assert np.array_equal(chain, hist(2, {1: 2})) and np.array_equal(delay, hist(5, {0: 1, 4: 2}))
    # counts are added to what the bins hold, as a uint64_t
    start = np.array([1, (1 << 32) - 1, 1 << 40, (1 << 64) - 1, 0], np.uint64)
    want = np.array([2, (1 << 32) - 1, 1 << 40, (1 << 64) - 1, 2], np.uint64)
    assert np.array_equal(metrics_ref.bins(delays, 5, start), want) and start[0] == 1


# ------------------------------------------------------------------ the CPU oracle's executor
def former_oracle_hists(planes, order, release, nexec, nbc, nbd):
    """What test_gpu_parity.oracle_hists computed before it moved onto metrics_ref, word for word."""
    chain = np.zeros(nbc, np.uint64)
    delay = np.zeros(nbd, np.uint64)
    t = planes.hdr & 0xFFFFFF
    for s in range(planes.S):
        k = int(nexec[s])
        if not k:
            continue
        o = order[_lib.index(np.arange(k), s, planes.steps)]
        rec = (o & 0x7FFFFFFF).astype(np.int64)
        start = (o & _lib.FX_ORDER_SCC_START) != 0
        rel = release[_lib.index(rec, s, planes.steps)].astype(np.int64)
        d = t[_lib.index(rel, s, planes.steps)].astype(np.int64) - t[_lib.index(rec, s, planes.steps)]
        np.add.at(delay, np.minimum(d, nbd - 1), 1)
        starts = np.flatnonzero(start)
        sizes = np.diff(np.append(starts, k))
        np.add.at(chain, np.minimum(sizes, nbc - 1), 1)
    return chain, delay


@pytest.mark.parametrize("seed,case", [(11, dict(n=5, instances=40, cmds=200, window=8, cycle_pct=30)),
                                       (12, dict(n=2, instances=33, cmds=77, window=5, cycle_pct=40))])
def test_restatement_matches_the_oracle_executor(seed, case):
    planes_ = fs.synth_host(fs.synth_params(seed=seed, **case))
    order, release, nexec, err = oracle_lib.batch_execute(planes_, threads=4)
    assert np.all(err == 0) and np.all(nexec == planes_.steps)
    for nbc, nbd in ((64, 2048), (4, 16)):
        want = former_oracle_hists(planes_, order, release, nexec, nbc, nbd)
        got = metrics_ref.hists(planes_.hdr, order, release, nexec, planes_.S, planes_.steps, nbc, nbd)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert int(got[1].sum()) == planes_.S * planes_.steps and got[0][2:].sum() > 0  # SCCs of several rows too
    from test_gpu_parity import oracle_hists  # the old name, where the GPU tests import it from
    assert all(np.array_equal(a, b) for a, b in zip(oracle_hists(planes_, order, release, nexec, 64, 2048),
                                                    former_oracle_hists(planes_, order, release, nexec, 64, 2048)))


# ------------------------------------------------------------------ every case sits on its edge
def by_name(name, pair=E.PAIRS[1]):
    return E.case(name, *pair)


def test_the_bin_pairs_sit_on_the_lds_limit():
    assert [E.lds_bytes(*p) for p in E.PAIRS] == [16, 16640, 48 * 1024, 48 * 1024 + 4]
    assert [E.uses_lds(*p) for p in E.PAIRS] == [True, True, True, False]
    assert E.PAIRS == [(2, 2), (64, 4096), (64, 12224), (64, 12225)]


def test_block_counts_and_grids():
    want = {"narrow tails 1x1": (1, 1, False), "narrow tails 1x3": (1, 1, False), "narrow tails 3x5": (1, 1, False),
            "narrow tails 5x7": (1, 1, False), "narrow tails 63x4": (1, 1, False),
            "narrow tails 64x28": (7, 7, False), "narrow tails 64x32": (8, 8, True),
            "narrow tails 1x2048": (8, 8, True),
            "narrow / tiled 64x40": (10, 10, False), "narrow / tiled 65x40": (20, 20, False),
            "narrow / tiled 129x9": (9, 9, False), "narrow / tiled 130x9": (9, 9, False),
            "stride 64x8197": (2050, 2048, True), "stride 65x4101": (2052, 2048, False),
            "empty 0x8": (0, 0, False), "empty 8x0": (0, 0, False)}
    for name, (blocks, grid, permuted) in want.items():
        c = by_name(name)
        assert (E.blocks(c.S, c.steps), E.grid(c.S, c.steps), E.permuted(c.S, c.steps)) == (blocks, grid, permuted), name
    # tails: the last narrow block is not full (63x4: 252 of 256 words; 3x5: 24), steps % 4 != 0 among them
    assert all(4 * S * ((steps + 3) // 4) % 256 != 0 for S, steps in ((1, 1), (1, 3), (3, 5), (5, 7), (63, 4)))
    assert by_name("rows that do not count 6x21").steps % 4 == 1


def test_the_same_streams_on_either_side_of_64():
    for lo, hi, extra in (("narrow / tiled 64x40", "narrow / tiled 65x40", [64]),
                          ("narrow / tiled 129x9", "narrow / tiled 130x9", [129])):
        a, b = by_name(lo), by_name(hi)
        for s in range(a.S):
            rows = np.arange(a.steps)
            for name in ("hdr", "order", "release"):
                assert np.array_equal(getattr(a, name)[a.at(rows, s)], getattr(b, name)[b.at(rows, s)])
        assert np.array_equal(a.nexec, b.nexec[:a.S])
        rest = metrics_ref.hists(b.hdr, b.order, b.release, b.nexec, b.S, b.steps, 64, 4096, extra)
        assert all(np.array_equal(x + y, z) for x, y, z in zip(a.expected(64, 4096), rest, b.expected(64, 4096)))
        assert rest[1].sum() > 0


def test_stride_cases_keep_two_bins_for_the_late_blocks():
    for name, counts in (("stride 64x8197", (64 * 4, 64 * 1)), ("stride 65x4101", (4 + 4, 4 + 1))):
        c = by_name(name)
        delays, _ = c.samples()
        assert len(delays) == c.S * c.steps  # every row gives a sample
        assert tuple(int(np.sum(delays == d)) for d in E.SPECIAL) == counts
        # and they come from the rows of the blocks from 2048 on
        late = E.Case("late", c.S, c.steps)
        late.hdr, late.order, late.release, late.nexec = c.hdr, c.order.copy(), c.release, c.nexec
        for s in range(c.S):
            k = np.arange(c.steps)
            blk = k // 4 if c.S == 64 else (s // 64) * ((c.steps + 3) // 4) + k // 4
            late.order[late.at(k[blk >= E.MAX_GRID], s)] = 0x7FFFFFFF  # rows that give nothing
        left, _ = late.samples()
        assert len(delays) - len(left) == sum(counts) and not np.any(np.isin(left, E.SPECIAL))


@pytest.mark.parametrize("nbc,nbd", E.PAIRS)
def test_clamp_cases_reach_the_last_bin_and_the_one_below(nbc, nbd):
    _, delay = E.case("delay clamp 4x16", nbc, nbd).expected(nbc, nbd)
    assert delay[nbd - 1] >= 1 and delay[nbd - 2] >= 1
    delays, _ = E.case("delay clamp 4x16", nbc, nbd).samples()
    assert {nbd - 2, nbd - 1, nbd, 0, 0xFFFFFF, (1 << 32) - 1, (1 << 32) - 0xFFFFFF} <= set(int(d) for d in delays)
    sizes = np.concatenate([E.case(n, nbc, nbd).samples()[1] for n in ("chain clamp a 3x(nbc+6)",
                                                                         "chain clamp b 3x(nbc+6)")])
    assert {nbc - 1, nbc, nbc + 3, nbc + 6, 3} <= set(int(z) for z in sizes)
    chain = sum(E.case(n, nbc, nbd).expected(nbc, nbd)[0] for n in ("chain clamp a 3x(nbc+6)",
                                                                   "chain clamp b 3x(nbc+6)"))
    assert chain[nbc - 1] >= 1
    if nbc > 2:  # no SCC has 0 rows: with two bins the one below the last stays empty
        assert nbc - 2 in sizes and chain[nbc - 2] >= 1
    else:
        assert chain[0] == 0
    b = E.case("chain clamp b 3x(nbc+6)", nbc, nbd)
    above = b.order[b.at(np.arange(int(b.nexec[2]), b.steps), 2)]
    assert len(above) == 2 and not np.any(above & FLAG)  # only the count ends that SCC


def test_chain_rows_start_where_they_should():
    c = by_name("chain rows 3x260")
    starts = lambda s: list(np.flatnonzero(c.order[c.at(np.arange(260), s)] & FLAG))
    assert starts(0) == [3, 4, 255, 256] and starts(1) == [0, 3, 8, 255, 257] and starts(2) == [0, 4, 255]
    assert sorted(c.samples()[1]) == sorted([1, 251, 1, 4, 3, 5, 247, 2, 3, 4, 251, 5])
    # narrow mapping: word 4 S (k // 4) + 4 s + k % 4; row 255 of stream 2 ends a 256-thread block
    assert 12 * (255 // 4) + 4 * 2 + 255 % 4 == 3 * 256 - 1


def test_wave_extremes():
    one = by_name("one bin 64x64")
    assert set(one.samples()[0]) == {5} and set(one.samples()[1]) == {1} and len(one.samples()[0]) == 64 * 64
    every = by_name("all bins 64x64")
    assert sorted(set(every.samples()[0])) == list(range(64)) and set(every.samples()[1]) == set(range(1, 8))
    for name in ("all bins of a wave 64x64", "all bins of a wave 65x64"):
        c = by_name(name)
        for s0 in range(0, 64, 16):  # a wave: 16 streams by the 4 rows of a block, in either mapping
            got = {int(c.hdr[c.at(63, s)] & 0xFFFFFF) - int(c.hdr[c.at(k, s)] & 0xFFFFFF)
                   for s in range(s0, s0 + 16) for k in (60, 61, 62, 3)}  # order row 63 names arrival 3
            assert got == set(range(64))


def test_rows_that_do_not_count():
    c = by_name("rows that do not count 6x21")
    assert [int(x) for x in c.nexec] == [0, 1, 21, 21, 21, 22]
    per = [metrics_ref.samples(c.hdr, c.order, c.release, c.nexec, c.S, c.steps, [s]) for s in range(6)]
    assert [len(d) for d, _ in per] == [0, 1, 21, 16, 16, 0]
    assert sorted(per[3][1]) == [2] and sorted(per[4][1]) == [10, 11]
    fixed = c.nexec.copy()
    fixed[5] = 21  # what an unguarded pass would take from stream 5: 21 samples
    assert len(metrics_ref.samples(c.hdr, c.order, c.release, fixed, c.S, c.steps, [5])[0]) == 21
    assert np.all(c.order[c.at(np.arange(1, 21), 1)] == E.A5) and np.all(c.order[c.at(np.arange(21), 0)] == E.A5)
    assert max(int(x) for x in c.nexec) <= c.steps + 3


def test_no_case_counts_beyond_the_pad_rows():
    for pair in E.PAIRS:
        for c in E.all_cases(*pair):
            assert all(int(x) <= c.steps + 3 or c.steps == 0 for x in c.nexec), c.name
            assert len(c.hdr) == len(c.order) == len(c.release) == _lib.plane_words(c.S, c.steps)
