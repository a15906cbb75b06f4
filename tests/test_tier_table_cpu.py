"""What the library says about its executor tiers, against values recorded from
the build before the tiers were described in one table (tests/golden/tier_table.json):
fx_tier_query's status and four fields and fx_batch_state_bytes, for every tier
and one past the last.  The query writes into a struct prefilled with
0xFFFFFFFF, so a tier it refuses without writing shows as that.  CPU only.

    python tests/test_tier_table_cpu.py      # rewrites the recorded values"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

from fantoch_amd import _lib  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "tier_table.json")
TIERS = range(_lib.FX_NUM_TIERS + 1)
QUERY_N = list(range(1, 10)) + [16, 17]
BYTES_N = (1, 5, 8)
LANES = (0, 1, 63, 64, 65, 300)
FILL = 0xFFFFFFFF


def measured():
    lib = _lib.load()
    query, state = {}, {}
    for tier in TIERS:
        for n in QUERY_N:
            info = _lib.TierInfo(FILL, FILL, FILL, FILL)
            st = lib.fx_tier_query(tier, n, ctypes.byref(info))
            query["%d,%d" % (tier, n)] = [st, info.max_sources, info.pending_cap, info.window_bits, info.state_words]
        for n in BYTES_N:
            for lanes in LANES:
                state["%d,%d,%d" % (tier, n, lanes)] = lib.fx_batch_state_bytes(tier, n, lanes)
    return {"fx_tier_query": query, "fx_batch_state_bytes": state}


def recorded():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_every_case_is_recorded():
    rec = recorded()
    assert len(rec["fx_tier_query"]) == len(TIERS) * len(QUERY_N)
    assert len(rec["fx_batch_state_bytes"]) == len(TIERS) * len(BYTES_N) * len(LANES)


def test_tier_query_is_as_recorded():
    got, want = measured()["fx_tier_query"], recorded()["fx_tier_query"]
    assert {k: v for k, v in got.items() if v != want.get(k)} == {}
    assert got.keys() == want.keys()


def test_state_bytes_are_as_recorded():
    got, want = measured()["fx_batch_state_bytes"], recorded()["fx_batch_state_bytes"]
    assert {k: v for k, v in got.items() if v != want.get(k)} == {}
    assert got.keys() == want.keys()


def test_query_refuses_a_null_struct():
    assert _lib.load().fx_tier_query(0, 3, None) == _lib.FX_ERR_INVALID_ARG


if __name__ == "__main__":
    with open(GOLDEN, "w") as fh:
        json.dump(measured(), fh, indent=0, sort_keys=True)
        fh.write("\n")
