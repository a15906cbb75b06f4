"""Restatement of fx_kv_monitor_compare (check_monitors over pairs of streams)
from the header's wording alone, in plain Python: which pairs cannot be
compared, and kv_ref.first_difference over the per-key sequences of the rest.

A side is anything with num_streams, steps, keys and three readers:
off(s, k) = mon_off[s][k], row(s, r) = the monitor's row r of stream s,
word(s, a) = the rifl word of arrival row a of stream s.  Plain is such a side
over nested lists, for answers written out by hand."""
import kv_ref

AGREE = (0xFFFFFFFF, 0xFFFFFFFF)  # (FX_KV_AGREE, FX_KV_AGREE)
BAD = (0xFFFFFFFE, 0xFFFFFFFE)    # (FX_KV_BAD_PAIR, FX_KV_BAD_PAIR)


class Plain:
    """mon_off[s] = keys + 1 offsets, monitor[s] = arrival rows by monitor row, rifl[s] = words by arrival row."""

    def __init__(self, steps, keys, mon_off, monitor, rifl):
        self.num_streams, self.steps, self.keys = len(mon_off), steps, keys
        self.mon_off, self.monitor, self.rifl = mon_off, monitor, rifl

    def off(self, s, k):
        return self.mon_off[s][k]

    def row(self, s, r):
        return self.monitor[s][r]

    def word(self, s, a):
        return self.rifl[s][a]


def why_not(m, s):
    """None if stream s of side m can be compared, else the first rule it breaks:
    ("stream",), ("first",), ("descending", k) for mon_off[k] > mon_off[k + 1], ("end",) or
    ("row", r) for the first monitor row in use that names no arrival row."""
    if not 0 <= s < m.num_streams:
        return ("stream",)
    off = [m.off(s, k) for k in range(m.keys + 1)]
    if off[0] != 0:
        return ("first",)
    for k in range(m.keys):
        if off[k] > off[k + 1]:
            return ("descending", k)
    if off[m.keys] > m.steps:
        return ("end",)
    for r in range(off[m.keys]):
        if m.row(s, r) >= m.steps:
            return ("row", r)
    return None


def sequences(m, s):
    """({key: [arrival rows]}, {arrival row: rifl word}) of a stream that can be compared."""
    mon = {k: [m.row(s, r) for r in range(m.off(s, k), m.off(s, k + 1))] for k in range(m.keys)}
    return mon, {a: m.word(s, a) for rows in mon.values() for a in rows}


def compare(side_a, sa, side_b, sb):
    """(key, pos), AGREE or BAD for the pair (stream sa of side_a, stream sb of side_b)."""
    assert side_a.keys == side_b.keys
    if why_not(side_a, sa) is not None or why_not(side_b, sb) is not None:
        return BAD
    mon_a, rifl_a = sequences(side_a, sa)
    mon_b, rifl_b = sequences(side_b, sb)
    d = kv_ref.first_difference(mon_a, rifl_a, mon_b, rifl_b, side_a.keys)
    return AGREE if d is None else d
