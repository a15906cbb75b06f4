"""Hand-built monitors for fx_kv_monitor_compare (k_kv_compare, kv_exec.hip), one case per edge of the kernel,
shared by the CPU and the GPU tests.  No executor runs: a Side is the monitor plane, the mon_off rows and the rifl
plane of a batch as fx_kv_execute could have left them, or, after a corruption, as it never would.  Every word a
call must not read holds 0xA5A5A5A5: monitor rows at or above mon_off[s][keys], the rifl rows no monitor row
names, pad rows, pad streams and the mon_off rows of streams that were not given (streams that ended with an
error).  The expected answers come from the restatement (monitor_ref), whose own answers
test_monitor_edges_ref.py pins; where a case knows its answer by construction it states it, and the same file
holds the restatement to it.

A spec is {key: [rifl words]}: the commands executed on each key, in order.  word(k, i) names command i of key
k, other(k, i) another command in its place; no two are equal and none is the fill, so a read through a wrong
index (another row, stream or side) shows as a difference.  place() gives every command an arrival row, and the
two sides of a case differ in S, in steps and in the placement, so the two fx_index strides differ and the same
command sits at different arrival rows.  Every case also runs with its sides swapped and each pair reversed."""
import functools
import math

import numpy as np

import monitor_ref
from fantoch_amd import _lib
from fantoch_amd import kv as K

A5 = 0xA5A5A5A5
AGREE, BAD = "AGREE", "BAD"  # kinds of answer; a position is written as (key, pos), or POS where only the kind is stated
POS = "POS"
ABOVE = _lib.FX_KV_ONCHIP_KEYS + 88
FAR = (1 << 31) | 5  # a stream index far above any set


def word(k, i):
    return 0x01000000 + (k << 12) + i


def other(k, i):
    return word(k, i) | 0x40000000


class Side:
    """One fx_kv_monitor.  streams: {s: {key: [(arrival row, rifl word), ...]}}."""

    def __init__(self, S, steps, keys, streams):
        self.S = self.num_streams = S
        self.steps, self.keys = steps, keys
        self.plane = _lib.plane_words(S, steps)
        self.monitor, self.rifl = np.full(self.plane, A5, np.uint32), np.full(self.plane, A5, np.uint32)
        self.mon_off = np.full((S, keys + 1), A5, np.uint32)
        for s, per_key in streams.items():
            assert 0 <= s < S and all(0 <= k < keys for k in per_key)
            r, seen = 0, set()
            for k in range(keys):
                self.mon_off[s, k] = r
                for a, w in per_key.get(k, []):
                    assert 0 <= a < steps and a not in seen and w != A5
                    seen.add(a)
                    self.monitor[_lib.index(r, s, steps)] = a
                    self.rifl[_lib.index(a, s, steps)] = w
                    r += 1
            assert r <= steps
            self.mon_off[s, keys] = r

    # the readers monitor_ref asks for
    def off(self, s, k):
        return int(self.mon_off[s, k])

    def row(self, s, r):
        return int(self.monitor[_lib.index(r, s, self.steps)])

    def word(self, s, a):
        return int(self.rifl[_lib.index(a, s, self.steps)])

    # corruptions
    def set_off(self, s, k, value):
        self.mon_off[s, k] = value

    def set_row(self, s, r, value):
        assert r < (self.steps + 3) // 4 * 4  # inside the stream's own rows of the plane, its pad rows included
        self.monitor[_lib.index(r, s, self.steps)] = value

    def arrays(self):
        return self.monitor, self.mon_off, self.rifl

    def result(self, dev=None):
        """The side as a KvResult (what compare_monitors and compare_monitors_host take)."""
        none = np.zeros(0, np.uint32)
        return K.KvResult(self.S, self.steps, self.keys, 1, none, np.zeros(self.S * self.keys, np.uint32), self.monitor,
                          self.mon_off, np.zeros(self.S, np.uint32), 0, dev)


class View:
    """The readers of monitor_ref over a KvResult and a rifl plane (monitors an executor wrote)."""

    def __init__(self, res, rifl):
        self.num_streams, self.steps, self.keys = res.S, res.steps, res.keys
        self.monitor, self.mon_off, self.rifl = res.monitor, res.mon_off, rifl

    off, row, word = Side.off, Side.row, Side.word


class Case:
    """Two sides, pairs (stream of a, stream of b) and per pair the kind of answer the case is built for: AGREE,
    BAD, POS or the position itself.  want: the restatement's answers."""

    def __init__(self, name, a, b, pairs, kinds):
        assert len(pairs) == len(kinds)
        self.name, self.a, self.b, self.pairs, self.kinds = name, a, b, [tuple(p) for p in pairs], list(kinds)
        self._want = None

    @property
    def want(self):
        if self._want is None:
            memo = {}
            for p in self.pairs:
                if p not in memo:
                    memo[p] = monitor_ref.compare(self.a, p[0], self.b, p[1])
            self._want = [memo[p] for p in self.pairs]
        return self._want

    def swapped(self):
        return Case(self.name + ", sides swapped", self.b, self.a, [(y, x) for x, y in self.pairs], self.kinds)


def kind_of(answer):
    return AGREE if answer == monitor_ref.AGREE else BAD if answer == monitor_ref.BAD else POS


# ------------------------------------------------------------------ specs
def spec(lengths):
    """lengths: {key: rows} or a list by key."""
    items = lengths.items() if isinstance(lengths, dict) else enumerate(lengths)
    return {k: [word(k, i) for i in range(n)] for k, n in items if n}


def total(sp):
    return sum(len(v) for v in sp.values())


def alter(sp, k, i):
    """Another command at position i of key k."""
    out = {key: list(v) for key, v in sp.items()}
    out[k][i] = other(k, i)
    return out


def locate(sp, r):
    """(key, position) of linear row r."""
    for k in sorted(sp):
        if r < len(sp[k]):
            return k, r
        r -= len(sp[k])
    raise IndexError(r)


def alter_rows(sp, *rows):
    for r in rows:
        sp = alter(sp, *locate(sp, r))
    return sp


def resize(sp, k, n):
    """Key k with n rows: cut, or continued with further commands of its own."""
    out = {key: list(v) for key, v in sp.items()}
    have = out.get(k, [])
    out[k] = have[:n] + [word(k, i) for i in range(len(have), n)]
    if not out[k]:
        del out[k]
    return out


def place(sp, steps, how):
    """Every command of the spec on an arrival row of its own: "up" in the order of the monitor, "down" from the
    last row backwards, "mixed" in strides over all rows."""
    n = total(sp)
    assert n <= steps
    if how == "up":
        rows = list(range(n))
    elif how == "down":
        rows = [steps - 1 - j for j in range(n)]
    else:
        m = next(p for p in (37, 41, 43, 47) if math.gcd(p, steps) == 1)
        rows = [(j * m + 11) % steps for j in range(n)]
    out, j = {}, 0
    for k in sorted(sp):
        out[k] = [(rows[j + i], w) for i, w in enumerate(sp[k])]
        j += len(sp[k])
    return out


def sides(keys, lefts, rights, a, b):
    """lefts / rights: {stream: spec}; a, b: (S, steps, placement); S None: one stream more than a needs and three
    more than b needs, streams that were never written."""
    out = []
    for specs, (S, steps, how) in ((lefts, a), (rights, b)):
        S = max(specs) + (2 if specs is lefts else 4) if S is None else S
        out.append(Side(S, steps, keys, {s: place(sp, steps, how) for s, sp in specs.items()}))
    return out


# ------------------------------------------------------------------ key strips
STRIP_KEYS = [1, 2, 63, 64, 65, 128, 129, ABOVE]


def strip_lengths(keys):
    """One row on every key below 140, on every eighth above and on the last."""
    return {k: 1 for k in range(keys) if k < 140 or k % 8 == 0 or k == keys - 1}


def strips(keys):
    """Stream 0 of a against streams of b that have one row more on some keys: the answer is (the smallest such
    key, 1).  The last variant has no row on the last key: (keys - 1, 0)."""
    base = spec(strip_lengths(keys))
    n = total(base)
    longer = [[kl] for kl in (0, 63, 64, 65, keys - 1)]
    longer += [[10, 69], [70, 3]]             # the larger key on a lower lane; on a higher one
    longer += [[69, 20], [5, 69], [130, 100]]  # a lane's second strip against another's first; one lane's two; third against second
    rights, kinds = {0: base}, [AGREE]
    for n_seen, ks in enumerate(longer):
        if max(ks) < keys and ks not in longer[:n_seen]:
            sp = base
            for k in ks:
                sp = resize(sp, k, 2)
            rights[len(rights)] = sp
            kinds.append((min(ks), 1))
    rights[len(rights)] = resize(base, keys - 1, 0)
    kinds.append((keys - 1, 0))
    a, b = sides(keys, {0: base}, rights, (None, n + 1, "mixed"), (None, n + 2, "down"))
    return Case("key strips, %d keys" % keys, a, b, [(0, j) for j in range(len(kinds))], kinds)


# ------------------------------------------------------------------ row chunks
ROW_TOTALS = [0, 1, 63, 64, 65, 128, 129, "steps"]
FULL = 130  # the monitor that fills every row of its side: mon_off[keys] == steps


def chunks(rows):
    """7 keys, 3 of them in use.  Stream 0 of a against streams of b with other commands on chosen linear rows:
    rows 0, 63, 64, 65 and the last; two in different chunks of 64; two in one chunk."""
    full = rows == "steps"
    n = FULL if full else rows
    base = spec({0: n // 3, 2: n // 2, 5: n - n // 3 - n // 2})
    assert total(base) == n
    changes = [[0], [63], [64], [65], [n - 1], [10, 100], [70, 128], [128, 70], [66, 90], [6, 5]]
    rights, kinds = {0: base}, [AGREE]
    for n_seen, rs in enumerate(changes):
        if 0 <= min(rs) and max(rs) < n and rs not in changes[:n_seen]:
            rights[len(rights)] = alter_rows(base, *rs)
            kinds.append(locate(base, min(rs)))
    a, b = sides(7, {0: base}, rights, (None, n if full else n + 5, "mixed"), (None, n + 3 if full else n + 9, "down"))
    return Case("row chunks, %s rows" % rows, a, b, [(0, j) for j in range(len(kinds))], kinds)


# ------------------------------------------------------------------ length against content
def length_against_content():
    L = [3, 0, 4, 2, 5, 3, 0, 2]
    base = spec(L)
    lefts = {0: base,
             1: resize(base, 3, 0),   # a is the shorter side, with no row on the key
             2: resize(base, 4, 2)}   # a is the shorter side
    rights = {0: base,
              1: resize(base, 3, 3),                  # the same sequences behind key 3
              2: alter(resize(base, 3, 3), 5, 1),     # a content difference above kl is not reported
              3: alter(resize(base, 3, 3), 2, 1),     # one below kl beats it
              4: alter(resize(base, 4, 3), 4, 1),     # one inside kl below the shorter length
              5: resize(base, 3, 0),                  # b is the shorter side, with no row on the key
              6: alter(resize(base, 4, 3), 4, 2),     # the last common position of kl
              7: alter(resize(base, 3, 3), 3, 1),
              8: alter(resize(base, 3, 3), 3, 2)}     # beyond the shorter length: only the length counts
    pairs = [((0, 0), AGREE), ((0, 1), (3, 2)), ((0, 2), (3, 2)), ((0, 3), (2, 1)), ((0, 4), (4, 1)), ((0, 5), (3, 0)),
             ((0, 6), (4, 2)), ((0, 7), (3, 1)), ((0, 8), (3, 2)), ((1, 0), (3, 0)), ((1, 5), AGREE), ((1, 1), (3, 0)),
             ((2, 0), (4, 2)), ((2, 4), (4, 1)), ((2, 6), (4, 2)), ((2, 3), (2, 1))]
    a, b = sides(8, lefts, rights, (None, 23, "mixed"), (None, 29, "down"))
    return Case("length against content", a, b, [p for p, _ in pairs], [k for _, k in pairs])


# ------------------------------------------------------------------ the key of a linear row
SEARCH_KEYS = [1, 2, 37, ABOVE]


def search_lengths(keys, t, layout):
    if layout == "only":
        L = {}
    else:
        L = {k: 1 + k % 3 for k in range(keys)} if keys <= 40 else {k: 1 for k in range(0, keys, 5)}
        if layout == "island":  # runs of empty keys directly before and directly behind t
            for k in range(t - 5, t + 6):
                L.pop(k, None)
    L[t] = 3
    return L


def search(keys):
    """Stream j of a against stream j of b, which has another command on the first or on the last row of one key
    t: key 0, 1, the middle, keys - 2 and keys - 1; among keys that all hold rows, as the only key that does, and
    between runs of empty keys."""
    lefts, rights, kinds = {}, {}, []
    for t in sorted({0, 1, keys // 2, keys - 2, keys - 1} & set(range(keys))):
        for layout in ("dense", "only", "island"):
            for i in (0, 2):
                base = spec(search_lengths(keys, t, layout))
                lefts[len(lefts)] = base
                rights[len(rights)] = alter(base, t, i)
                kinds.append((t, i))
    n = max(total(sp) for sp in lefts.values())
    a, b = sides(keys, lefts, rights, (None, n + 2, "mixed"), (None, n + 5, "down"))
    return Case("search, %d keys" % keys, a, b, [(j, j) for j in range(len(kinds))], kinds)


# ------------------------------------------------------------------ two different batches
TWO_PAIRS = [((0, 63), AGREE), ((1, 64), (65, 0)), ((2, 65), (65, 1)), ((2, 0), AGREE), ((0, 2), (0, 0)),
             ((2, 1), (69, 1)), ((1, 5), (69, 1)), ((1, 0), AGREE)]


@functools.lru_cache(maxsize=None)
def two_sides():
    """a: 3 streams of 70 rows; b: 66 streams of 131 rows, the ones in use at 0, 1, 2, 5 and in the second tile
    of streams at 63 (the first tile's last), 64 and 65.  66 keys with one row and key 69 with two: 68 rows."""
    L = {k: 1 for k in range(66)}
    L[69] = 2
    base = spec(L)
    rights = {63: base, 64: alter_rows(base, 65), 65: resize(base, 65, 2), 0: base, 2: alter_rows(base, 0),
              1: alter(base, 69, 1), 5: resize(base, 69, 1)}
    return tuple(sides(70, {0: base, 1: base, 2: base}, rights, (3, 70, "mixed"), (66, 131, "down")))


def two_batches():
    a, b = two_sides()
    return Case("two different batches", a, b, [p for p, _ in TWO_PAIRS], [k for _, k in TWO_PAIRS])


# ------------------------------------------------------------------ pairs that cannot be compared
BAD_KEYS, BAD_STEPS, BAD_S = 129, 131, 24
BAD_LAST = 67  # the last monitor row in use
# stream of a -> (what is overwritten, the rule of monitor_ref.why_not it breaks).  mon_off[0] is 0 in every
# stream that passes the first rule, so no such stream has mon_off[0] > mon_off[1]: the decrease "at key 0" is
# key 0's end above key 1's end, mon_off[1] > mon_off[2].
CORRUPT = {
    1: ("mon_off[0] = 1", ("first",)),
    2: ("mon_off[1] above mon_off[2]", ("descending", 1)),
    3: ("mon_off[64] below mon_off[63]", ("descending", 63)),
    4: ("mon_off[65] below mon_off[64]", ("descending", 64)),
    5: ("mon_off[keys] below mon_off[keys - 1]", ("descending", BAD_KEYS - 1)),
    6: ("mon_off[keys] = steps + 1", ("end",)),
    7: ("monitor row 0 = steps", ("row", 0)),
    8: ("monitor row 0 = 0x7FFFFFFF", ("row", 0)),
    9: ("monitor row 64 = steps", ("row", 64)),
    10: ("monitor row 64 = 0x7FFFFFFF", ("row", 64)),
    11: ("monitor row 67 = steps", ("row", BAD_LAST)),
    12: ("monitor row 67 = 0x7FFFFFFF", ("row", BAD_LAST)),
    13: ("a mon_off row of 0xA5 bytes", ("first",)),
    # every row in use, and one more: the pad row `steps` of the plane holds an arrival row, so that nothing
    # but the offset itself tells
    16: ("mon_off[keys] = steps + 1 behind a full monitor", ("end",)),
}
BAD_FILL_ROW, BAD_CLEAN = 14, 15  # an out-of-range entry in the first unused monitor row; an untouched stream


def bad_pairs():
    """Every corruption on side a alone (the swapped case has it on side b alone).  Every BAD pair sits between
    one that agrees and one that differs at linear row 66."""
    L = {k: 1 for k in range(0, BAD_KEYS, 2)}
    L[5] = 3
    base = spec(L)
    assert total(base) == BAD_LAST + 1
    lefts = {s: base for s in range(BAD_S) if s != 13}
    lefts[16] = resize(base, 7, BAD_STEPS - BAD_LAST - 1)
    assert total(lefts[16]) == BAD_STEPS and BAD_STEPS % 4
    a, b = sides(BAD_KEYS, lefts, {0: base, 1: alter_rows(base, 66)}, (BAD_S, BAD_STEPS, "mixed"), (5, 140, "down"))
    steps = BAD_STEPS
    a.set_off(1, 0, 1)
    a.set_off(2, 1, a.off(2, 2) + 1)
    a.set_off(3, 64, a.off(3, 63) - 1)
    a.set_off(4, 65, a.off(4, 64) - 1)
    a.set_off(5, BAD_KEYS, a.off(5, BAD_KEYS - 1) - 1)
    a.set_off(6, BAD_KEYS, steps + 1)
    for s, (r, v) in zip(range(7, 13), [(r, v) for r in (0, 64, BAD_LAST) for v in (steps, 0x7FFFFFFF)]):
        a.set_row(s, r, v)
    a.set_off(16, BAD_KEYS, steps + 1)
    a.set_row(16, steps, 0)
    a.set_row(BAD_FILL_ROW, BAD_LAST + 1, steps)
    differ = locate(base, 66)
    pairs = []
    for s in sorted(CORRUPT):
        pairs += [((0, 0), AGREE), ((s, 0), BAD), ((BAD_CLEAN, 1), differ)]
    pairs += [((BAD_S, 0), BAD), ((BAD_FILL_ROW, 0), AGREE), ((FAR, 0), BAD), ((BAD_FILL_ROW, 1), differ),
              ((BAD_S, 77), BAD), ((BAD_CLEAN, 0), AGREE), ((7, 1), BAD), ((BAD_S - 1, 1), differ)]
    return Case("pairs that cannot be compared", a, b, [p for p, _ in pairs], [k for _, k in pairs])


# ------------------------------------------------------------------ the launch
NUM_PAIRS = [0, 1, 2, 65, 300]


def launch(n):
    a, b = two_sides()
    rows = [TWO_PAIRS[i % len(TWO_PAIRS)] for i in range(n)]
    return Case("launch of %d pairs" % n, a, b, [p for p, _ in rows], [k for _, k in rows])


def repeated():
    a, b = two_sides()
    return Case("one pair 300 times", a, b, [TWO_PAIRS[1][0]] * 300, [TWO_PAIRS[1][1]] * 300)


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [strips(keys) for keys in STRIP_KEYS] + [chunks(rows) for rows in ROW_TOTALS]
    cases += [length_against_content()] + [search(keys) for keys in SEARCH_KEYS]
    cases += [two_batches(), bad_pairs()] + [launch(n) for n in NUM_PAIRS] + [repeated()]
    return tuple(cases + [c.swapped() for c in cases])


NAMES = [c.name for c in all_cases()]
IDS = [n.replace(", ", "-").replace(" ", "_") for n in NAMES]


def case(name):
    return all_cases()[NAMES.index(name)]


def facts(c, i):
    """Where pair i of a case sits, from the sides' arrays: kl (the first key whose lengths differ, or None), row
    (the first linear row below the kernel's limit whose commands differ, or None), rows (side a's rows in use).
    None for a pair that cannot be compared."""
    sa, sb = c.pairs[i]
    if monitor_ref.why_not(c.a, sa) or monitor_ref.why_not(c.b, sb):
        return None
    oa, ob = [int(x) for x in c.a.mon_off[sa]], [int(x) for x in c.b.mon_off[sb]]
    kl = next((k for k in range(c.a.keys) if oa[k + 1] - oa[k] != ob[k + 1] - ob[k]), None)
    limit = oa[-1] if kl is None else oa[kl] + min(oa[kl + 1] - oa[kl], ob[kl + 1] - ob[kl])
    row = next((r for r in range(limit) if c.a.word(sa, c.a.row(sa, r)) != c.b.word(sb, c.b.row(sb, r))), None)
    return dict(kl=kl, row=row, rows=oa[-1], limit=limit)
