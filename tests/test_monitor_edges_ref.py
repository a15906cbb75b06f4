"""The restatement of fx_kv_monitor_compare (monitor_ref) and the edge cases built on it (monitor_edges), before
either side of the library is asked anything: answers written out by hand for every rule of a pair that cannot
be compared and for every way a length and a content difference meet, and that every case sits on the edge it is
named after.  CPU only."""
import numpy as np
import pytest

import monitor_edges as E
import monitor_ref as M
from fantoch_amd import _lib

AGREE, BAD = M.AGREE, M.BAD


def plain(steps, keys, *streams):
    """Streams as per-key lists of rifl words; the command of monitor row r arrived at row steps - 1 - r."""
    mon_off, monitor, rifl = [], [], []
    for per_key in streams:
        assert len(per_key) == keys
        words = [w for seq in per_key for w in seq]
        off = [0]
        for seq in per_key:
            off.append(off[-1] + len(seq))
        mon_off.append(off)
        monitor.append([steps - 1 - r for r in range(len(words))] + [0xA5A5A5A5] * (steps - len(words)))
        rifl.append([0xA5A5A5A5] * (steps - len(words)) + words[::-1])
    return M.Plain(steps, keys, mon_off, monitor, rifl)


# ------------------------------------------------------------------ known answers
def test_constants_are_the_header_s():
    assert AGREE == (_lib.FX_KV_AGREE,) * 2 and BAD == (_lib.FX_KV_BAD_PAIR,) * 2
    assert E.ABOVE == _lib.FX_KV_ONCHIP_KEYS + 88 == 600


def test_known_answers_content():
    m = plain(8, 3, [[1, 2, 3], [], [4, 5]], [[1, 2, 3], [], [4, 5]], [[1, 9, 3], [], [4, 8]], [[1, 2, 3], [], [4, 8]])
    assert M.compare(m, 0, m, 1) == AGREE and M.compare(m, 1, m, 1) == AGREE
    assert M.compare(m, 0, m, 2) == (0, 1) == M.compare(m, 2, m, 0)  # two differences: the first wins
    assert M.compare(m, 0, m, 3) == (2, 1) and M.compare(m, 2, m, 3) == (0, 1)
    # the sides are two batches: the same commands at other arrival rows of a side with other steps
    other = plain(5, 3, [[1, 2, 3], [], [4, 5]], [[], [], []])
    assert M.compare(m, 0, other, 0) == AGREE and M.compare(other, 0, m, 3) == (2, 1)
    assert M.compare(m, 0, other, 1) == (0, 0) == M.compare(other, 1, m, 0)
    assert M.compare(other, 1, other, 1) == AGREE  # no rows at all


def test_known_answers_length_against_content():
    base = [[1, 2, 3], [4, 5], [6, 7, 8], [9]]
    m = plain(12, 4, base,
              [[1, 2, 3], [4, 5, 10], [6, 7, 8], [9]],    # 1: the same sequences behind the key whose lengths differ
              [[1, 2, 3], [4, 5, 10], [6, 77, 8], [9]],   # 2: a content difference above that key is not reported
              [[1, 22, 3], [4, 5, 10], [6, 7, 8], [9]],   # 3: one below it beats it
              [[1, 2, 3], [44, 5, 10], [6, 7, 8], [9]],   # 4: one inside it, below the shorter length
              [[1, 2, 3], [], [6, 7, 8], [9]],            # 5: the shorter length is 0
              [[1, 2, 3], [4], [6, 7, 8], [9]])           # 6
    assert M.compare(m, 0, m, 1) == (1, 2) == M.compare(m, 1, m, 0)
    assert M.compare(m, 0, m, 2) == (1, 2)
    assert M.compare(m, 0, m, 3) == (0, 1)
    assert M.compare(m, 0, m, 4) == (1, 0)
    assert M.compare(m, 0, m, 5) == (1, 0) == M.compare(m, 5, m, 0)  # b the shorter side, then a
    assert M.compare(m, 0, m, 6) == (1, 1) == M.compare(m, 6, m, 0)
    assert M.compare(m, 6, m, 4) == (1, 0) and M.compare(m, 5, m, 4) == (1, 0) and M.compare(m, 6, m, 1) == (1, 1)


def test_known_answers_pairs_that_cannot_be_compared():
    steps = 6
    good = plain(steps, 2, [[1, 2], [3]])

    def broken(**kw):
        m = plain(steps, 2, [[1, 2], [3]], [[1, 2], [3]])
        for name, (i, v) in kw.items():
            getattr(m, name)[0][i] = v
        return m

    assert M.compare(good, 0, good, 0) == AGREE
    cases = [(broken(mon_off=(0, 1)), ("first",)),
             (broken(mon_off=(1, 4)), ("descending", 1)),
             (broken(mon_off=(2, steps + 1)), ("end",)),
             (broken(monitor=(0, steps)), ("row", 0)),
             (broken(monitor=(2, 0x7FFFFFFF)), ("row", 2))]
    for m, rule in cases:
        assert M.why_not(m, 0) == rule and M.why_not(m, 1) is None
        assert M.compare(m, 0, good, 0) == BAD == M.compare(good, 0, m, 0), rule  # on side a alone, on side b alone
        assert M.compare(m, 1, good, 0) == AGREE == M.compare(good, 0, m, 1)      # the stream beside it is not touched
    assert M.why_not(good, 1) == ("stream",) == M.why_not(good, 1 << 31)
    assert M.compare(good, 1, good, 0) == BAD == M.compare(good, 0, good, 1)
    # legal: a monitor that fills every row, and anything in the first row that is not in use
    full = plain(3, 2, [[1, 2], [3]])
    assert full.mon_off[0][2] == full.steps and M.compare(full, 0, good, 0) == AGREE
    assert M.why_not(broken(monitor=(3, steps)), 0) is None and M.compare(broken(monitor=(3, steps)), 0, good, 0) == AGREE
    # a mon_off row as a stream with an error leaves it
    assert M.why_not(M.Plain(steps, 2, [[0xA5A5A5A5] * 3], [[0xA5A5A5A5] * steps], [[0xA5A5A5A5] * steps]), 0) == ("first",)


# ------------------------------------------------------------------ every case sits on its edge
ALL = E.all_cases()
PLAIN = [c for c in ALL if not c.name.endswith("swapped")]


def named(start):
    return [c for c in PLAIN if c.name.startswith(start)]


@pytest.mark.parametrize("name", E.NAMES, ids=E.IDS)
def test_every_pair_has_an_answer_of_the_kind_its_case_states(name):
    c = E.case(name)
    for p, kind, want in zip(c.pairs, c.kinds, c.want):
        if isinstance(kind, tuple):  # the position by construction
            assert want == kind, (name, p)
        else:
            assert E.kind_of(want) == kind, (name, p, want)


def test_swapped_cases_have_the_same_answers():
    half = len(ALL) // 2
    for c, d in zip(ALL[:half], ALL[half:]):
        assert d.name == c.name + ", sides swapped" and d.a is c.b and d.b is c.a
        assert d.pairs == [(y, x) for x, y in c.pairs] and d.want == c.want, c.name


def test_sizes_stay_small_and_the_sides_differ():
    for c in ALL:
        for m in (c.a, c.b):
            assert m.S <= 66 and m.steps <= 200 and m.keys <= E.ABOVE, c.name
            assert m.monitor.shape == m.rifl.shape == (_lib.plane_words(m.S, m.steps),) and m.mon_off.shape == (m.S, m.keys + 1)
        assert (c.a.S, c.a.steps) != (c.b.S, c.b.steps) and c.a.S != c.b.S and c.a.steps != c.b.steps, c.name


def test_everything_a_call_must_not_read_holds_the_fill():
    for c in PLAIN:
        for m in (c.a, c.b):
            named_rows, used = np.zeros(m.plane, bool), np.zeros(m.plane, bool)
            for s in range(m.S):
                if M.why_not(m, s) is None:
                    rows = _lib.index(np.arange(m.off(s, m.keys)), s, m.steps)
                    used[rows] = True
                    named_rows[_lib.index(m.monitor[rows].astype(np.int64), s, m.steps)] = True
            if c.name != "pairs that cannot be compared":  # whose corrupted streams hold rows nothing may follow
                assert np.all(m.monitor[~used] == E.A5), c.name
                assert np.all(m.rifl[~named_rows] == E.A5), c.name
            words = m.rifl[named_rows]
            assert not np.any(words == E.A5), c.name
            for s in range(m.S):  # distinct per command within a stream
                w = m.rifl[_lib.index(np.arange(m.steps), s, m.steps)]
                w = w[w != E.A5]
                assert len(set(w.tolist())) == len(w), (c.name, s)


def test_key_strips_reach_their_edges():
    assert [c.a.keys for c in named("key strips")] == [1, 2, 63, 64, 65, 128, 129, E.ABOVE]
    kls = {}
    for c in named("key strips"):
        kls[c.a.keys] = [E.facts(c, i)["kl"] for i in range(len(c.pairs))]
        assert all(E.facts(c, i)["row"] is None for i in range(len(c.pairs))), c.name  # lengths alone
        assert c.a.keys - 1 in kls[c.a.keys] and 0 in kls[c.a.keys] and None in kls[c.a.keys]
    assert {0, 63, 64, 65, 128} <= set(kls[129]) and {0, 63, 64, 65, E.ABOVE - 1} <= set(kls[E.ABOVE])
    # two keys with other lengths: (10, 69), (70, 3), a second strip against a first, one lane's two strips, third
    # against second
    big = E.case("key strips, 600 keys")
    two = []
    for i, (sa, sb) in enumerate(big.pairs):
        differ = [k for k in range(big.a.keys) if big.a.off(sa, k + 1) - big.a.off(sa, k) !=
                  big.b.off(sb, k + 1) - big.b.off(sb, k)]
        if len(differ) == 2:
            two.append(tuple(differ))
            assert big.want[i] == (differ[0], 1)
    assert two == [(10, 69), (3, 70), (20, 69), (5, 69), (100, 130)]
    assert 69 % 64 < 10 and 70 % 64 > 3 and 69 % 64 < 20 and 130 % 64 < 100 % 64  # the lanes that find them


def test_row_chunks_reach_their_edges():
    cases = named("row chunks")
    assert [E.facts(c, 0)["rows"] for c in cases] == [0, 1, 63, 64, 65, 128, 129, E.FULL]
    full = cases[-1]
    assert full.a.steps == E.FULL and full.a.off(0, full.a.keys) == full.a.steps  # every row in use: legal
    assert M.why_not(full.a, 0) is None
    for c in cases:
        rows = E.facts(c, 0)["rows"]
        got = [E.facts(c, i)["row"] for i in range(len(c.pairs))]
        assert all(E.facts(c, i)["kl"] is None for i in range(len(c.pairs))), c.name  # content alone
        assert set(got) >= {r for r in (0, 63, 64, 65, rows - 1) if 0 <= r < rows} | {None}, c.name
    # two differences: in other chunks (either order of making them), in one chunk; the first wins
    c = E.case("row chunks, 129 rows")
    got = [E.facts(c, i)["row"] for i in range(len(c.pairs))]
    assert got == [None, 0, 63, 64, 65, 128, 10, 70, 70, 66, 5]
    assert c.want[7] == c.want[8] == E.locate(E.spec({0: 43, 2: 64, 5: 22}), 70)


def test_length_against_content_reaches_every_bullet():
    c = E.case("length against content")
    f = [E.facts(c, i) for i in range(len(c.pairs))]
    seen = {(x["kl"], x["row"] is not None, w) for x, w in zip(f, c.want)}
    assert (3, False, (3, 2)) in seen   # the same sequences behind kl; a difference above it
    assert (3, True, (2, 1)) in seen    # one below kl
    assert (4, True, (4, 1)) in seen    # inside kl, below the shorter length
    assert (3, False, (3, 0)) in seen   # the shorter length is 0
    a_len = lambda sa, k: c.a.off(sa, k + 1) - c.a.off(sa, k)
    b_len = lambda sb, k: c.b.off(sb, k + 1) - c.b.off(sb, k)
    shorter = {("a" if a_len(sa, x["kl"]) < b_len(sb, x["kl"]) else "b", min(a_len(sa, x["kl"]), b_len(sb, x["kl"])))
               for (sa, sb), x in zip(c.pairs, f) if x["kl"] is not None}
    assert {("a", 0), ("b", 0), ("a", 2), ("b", 3)} <= shorter


def test_search_cases_reach_their_edges():
    assert [c.a.keys for c in named("search")] == [1, 2, 37, E.ABOVE]
    for c in named("search"):
        keys = c.a.keys
        lengths = lambda j: [c.a.off(j, k + 1) - c.a.off(j, k) for k in range(keys)]
        where = set()
        for j, (t, i) in enumerate(c.want):
            L = lengths(j)
            assert L[t] == 3 and i in (0, 2)
            only = sum(L) == 3
            before = t > 0 and not any(L[max(t - 5, 0):t])
            behind = t < keys - 1 and not any(L[t + 1:t + 6])
            where.add((t, i, "only" if only else "island" if before or behind else "dense"))
            f = E.facts(c, j)
            assert f["kl"] is None and f["row"] == sum(L[:t]) + i
        for t in {0, keys - 1}:
            for i in (0, 2):  # the first and the last row of the key
                assert (t, i, "only") in where, (c.name, t, i)
                if keys >= 37:
                    assert (t, i, "island") in where and (t, i, "dense") in where, (c.name, t, i)
        if keys >= 37:
            assert (keys // 2, 0, "island") in where and (keys // 2, 2, "only") in where


def test_two_batches_differ_in_every_stride():
    c = E.case("two different batches")
    assert (c.a.S, c.a.steps, c.b.S, c.b.steps) == (3, 70, 66, 131)
    assert all(sa != sb for sa, sb in c.pairs) and {63, 64, 65} <= {sb for _, sb in c.pairs}
    assert {E.kind_of(w) for w in c.want} == {E.AGREE, E.POS}
    # the same commands at other arrival rows, and rows of b that are no rows of a
    assert c.want[0] == AGREE and [c.a.row(0, r) for r in range(68)] != [c.b.row(63, r) for r in range(68)]
    assert max(c.b.row(63, r) for r in range(68)) >= c.a.steps
    rows = [E.facts(c, i) for i in range(len(c.pairs))]
    assert {x["row"] for x in rows} >= {0, 65, 67} and {x["kl"] for x in rows} >= {65, 69}


def test_bad_pairs_reach_every_rule_on_either_side():
    c = E.case("pairs that cannot be compared")
    d = E.case("pairs that cannot be compared, sides swapped")
    assert (c.a.keys, c.a.steps, c.a.S) == (E.BAD_KEYS, E.BAD_STEPS, E.BAD_S)
    for s, (what, rule) in E.CORRUPT.items():
        assert M.why_not(c.a, s) == rule, what
    assert {rule for _, rule in E.CORRUPT.values()} == {("first",), ("end",), ("descending", 1), ("descending", 63),
                                                       ("descending", 64), ("descending", 128), ("row", 0), ("row", 64),
                                                       ("row", 67)}
    assert [c.a.row(s, r) for s, r in ((7, 0), (9, 64), (11, 67))] == [c.a.steps] * 3
    assert [c.a.row(s, r) for s, r in ((8, 0), (10, 64), (12, 67))] == [0x7FFFFFFF] * 3
    assert c.a.off(6, c.a.keys) == c.a.steps + 1 and np.all(c.a.mon_off[13] == E.A5)
    assert c.a.off(16, c.a.keys) == c.a.steps + 1 and c.a.off(16, c.a.keys - 1) == c.a.steps - 1
    assert all(c.a.row(16, r) < c.a.steps for r in range(c.a.steps + 1))  # the pad row too: the offset alone tells
    assert c.a.off(0, c.a.keys) == 68 and c.a.row(E.BAD_FILL_ROW, 68) == c.a.steps and M.why_not(c.a, E.BAD_FILL_ROW) is None
    assert all(M.why_not(c.b, s) is None for s in (0, 1))  # side b is whole: the corruption is on one side alone
    assert (E.BAD_S, 0) in c.pairs and (E.FAR, 0) in c.pairs and (0, E.FAR) in d.pairs
    for s in E.CORRUPT:  # between a pair that agrees and one that differs
        i = c.pairs.index((s, 0))
        assert [E.kind_of(w) for w in c.want[i - 1:i + 2]] == [E.AGREE, E.BAD, E.POS]
        assert d.pairs[i] == (0, s) and d.want[i] == BAD
    # every index a call may form stays inside the buffers: offsets it may follow end at steps at the most
    for s in range(c.a.S):
        if M.why_not(c.a, s) in (None, ("row", 0), ("row", 64), ("row", 67)):
            assert c.a.off(s, c.a.keys) <= c.a.steps


def test_launch_sizes():
    assert [len(c.pairs) for c in named("launch of")] == E.NUM_PAIRS == [0, 1, 2, 65, 300]
    c = E.case("one pair 300 times")
    assert len(set(c.pairs)) == 1 and len(c.pairs) == 300 and E.kind_of(c.want[0]) == E.POS


def test_coverage_over_all_cases():
    """Each first key whose lengths differ, each differing linear row and each kind of answer appears."""
    kls, rows, last = set(), set(), 0
    for c in PLAIN:
        for i in range(len(c.pairs)):
            f = E.facts(c, i)
            if f is not None:
                kls.add(f["kl"])
                rows.add(f["row"])
                last += f["row"] is not None and f["row"] == f["rows"] - 1
    assert {0, 63, 64, 65, 128, E.ABOVE - 1} <= kls and {0, 63, 64, 65} <= rows and last >= 5
