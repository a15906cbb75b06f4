"""Every byte the host twins of the two Tempo generators write
(fx_table_synth_generate_host, fx_table_group_synth_generate_host) for the
geometries of tests/table_synth_shapes.py and tests/table_group_synth_shapes.py,
as SHA-256 digests recorded in tests/golden/table_synth_digests.json.  The
comparison with the Python restatement (tests/test_table_synth_cpu.py,
tests/test_table_group_synth_cpu.py) decodes streams and looks at reached
rows; this one pins the buffers whole.  No GPU.

A digest covers, in this order: hdr, dot, clock, votes, nkeys (if the geometry
has the plane), lengths; for groups then route, targets and the word
steps_out.  Running this file (with the repository root on PYTHONPATH) records
them again -- only when the model itself is meant to change."""
import hashlib
import json
import os

import numpy as np
import pytest

from fantoch_amd import table as ft

import table_group_synth_shapes as TG
import table_synth_shapes as TS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_synth_digests.json")


def sha(buffers):
    h = hashlib.sha256()
    for b in buffers:
        b = np.ascontiguousarray(b)
        assert b.dtype == np.uint32
        h.update(b.tobytes())
    return h.hexdigest()


def stream_digest(name):
    p = ft.synth_table_host(TS.params(name))
    return sha([p.hdr, p.dot, p.clock, p.votes] + ([p.nkeys] if p.nkeys is not None else []) + [p.lengths])


def group_digest(name):
    p, route, targets, steps_out = ft.synth_table_groups_host(TG.params(name))
    return sha([p.hdr, p.dot, p.clock, p.votes, p.nkeys, p.lengths, route, targets, np.array([steps_out], np.uint32)])


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_geometry_is_recorded():
    want = recorded()
    assert sorted(want["streams"]) == sorted(TS.GEOMS) and sorted(want["groups"]) == sorted(TG.GEOMS)
    assert (want["stream_seed"], want["stream_base"]) == (TS.SEED, TS.BASE)
    assert (want["group_seed"], want["group_base"]) == (TG.SEED, TG.BASE)


@pytest.mark.parametrize("name", sorted(TS.GEOMS))
def test_stream_bytes(name):
    assert stream_digest(name) == recorded()["streams"][name]


@pytest.mark.parametrize("name", sorted(TG.GEOMS))
def test_group_bytes(name):
    assert group_digest(name) == recorded()["groups"][name]


if __name__ == "__main__":
    out = dict(stream_seed=TS.SEED, stream_base=TS.BASE, group_seed=TG.SEED, group_base=TG.BASE,
               streams={name: stream_digest(name) for name in sorted(TS.GEOMS)},
               groups={name: group_digest(name) for name in sorted(TG.GEOMS)})
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
