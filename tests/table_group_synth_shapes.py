"""Geometries of the seeded generator of closed-loop shard groups
(fx_table_group_synth_*) shared by tests/test_table_group_synth_cpu.py and
tests/test_table_group_synth_gpu.py: keyword arguments of
fantoch_amd.table.table_group_synth_params.  Together they cover 1 group and
65 groups of P = 3 (195 streams: four tiles, the last ragged; the second
wavefront has one live lane), P = 1 (no lists), P = 8 with keys = 2, kmax = 2
(the key pick exhausts the pool, lists over 7 shards), smax < P, (n, fast
quorum) = (3, 2), (5, 3), (7, 4), state on chip (onchip_p2: 2 * 16 * 5 + 5 =
165 words) and in scratch (scratch_p3: 3 * 33 * 5 + 5 = 500), (window, lag) =
(0, 0), (4, 6), (9, 3), (9, 9), (50, 80), msg_lag = 0, 3, 31, conflict rates 0,
100 and two rates split by conflict_block, and cmds = 0 and 1.  The stability
threshold of a geometry is Tempo's for f = 1, n // 2 + 1.
tests/cpp/table_group_synth_host_check.cpp runs the host twin over a copy of
GEOMS in C++ (its `geoms` table, in this order): a geometry changed here is
changed there.

The seed is one under which every group of every geometry runs to the end in
the closed loop (tests/test_table_group_synth_cpu.py::
test_the_groups_run_to_the_end).  That is a property of the seed, not of the
model: of the 1,112 streams of four seeds tried one keeps a partial waiting,
seed 20250311, g65_p3, group 2: the StableAtShard for key 5 of a
two-key command reaches shard 1 in the round between the command's two
attached events there, and in the restatement (tests/table_ref_ps.py) that
partial ends with missing_stable_shards 1."""
import functools

from fantoch_amd import table as ft

GEOMS = {
    "g1_p2_n3": dict(groups=1, shards=2, n=3, fast_quorum=2, keys=16, kmax=2, cmds=40, conflicts=(2,), window=4, lag=6,
                     msg_lag=3),
    "g65_p3": dict(groups=65, shards=3, n=5, fast_quorum=3, keys=16, kmax=2, cmds=20, conflicts=(2, 50),
                   conflict_block=32, window=4, lag=6, msg_lag=3),
    "p1": dict(groups=3, shards=1, n=5, fast_quorum=3, keys=16, kmax=2, cmds=40, conflicts=(0,), window=4, lag=6,
               msg_lag=0),
    "p3_keys1_w0": dict(groups=2, shards=3, n=3, fast_quorum=2, keys=1, kmax=3, cmds=40, conflicts=(2,), window=0,
                        lag=0, msg_lag=0),
    "p8_keys2": dict(groups=2, shards=8, n=3, fast_quorum=2, keys=2, kmax=2, cmds=30, conflicts=(2,), window=9, lag=3,
                     msg_lag=0),
    "p8_msg31": dict(groups=2, shards=8, n=3, fast_quorum=2, keys=2, kmax=2, cmds=30, conflicts=(2,), window=9, lag=9,
                     msg_lag=31),
    "smax2_p4_n7": dict(groups=2, shards=4, smax=2, n=7, fast_quorum=4, keys=8, kmax=2, cmds=40, conflicts=(100,),
                        window=4, lag=6, msg_lag=3),
    "onchip_p2": dict(groups=2, shards=2, n=5, fast_quorum=3, keys=16, kmax=2, cmds=40, conflicts=(100,), window=4,
                      lag=6, msg_lag=3),
    "scratch_p3": dict(groups=3, shards=3, n=5, fast_quorum=3, keys=33, kmax=3, cmds=40, conflicts=(2,), window=4,
                       lag=6, msg_lag=3),
    "late_p2": dict(groups=2, shards=2, n=5, fast_quorum=3, keys=16, kmax=2, cmds=40, conflicts=(2,), window=50, lag=80,
                    msg_lag=3),
    "cmds0": dict(groups=3, shards=2, n=5, fast_quorum=3, keys=16, kmax=2, cmds=0, conflicts=(2,), window=4, lag=6,
                  msg_lag=3),
    "cmds1": dict(groups=3, shards=3, n=5, fast_quorum=5, keys=16, kmax=2, cmds=1, conflicts=(2,), window=4, lag=6,
                  msg_lag=3),
}
SEED, BASE = 20250312, 1000
DELAY_BITS = 0xF8000000  # the delay field of an FX_TABLE_TARGET word


def params(name, **over):
    kw = dict(GEOMS[name], seed=SEED, group_base=BASE)
    kw.update(over)
    return ft.table_group_synth_params(**kw)


def threshold(name):
    return GEOMS[name]["n"] // 2 + 1


@functools.lru_cache(maxsize=None)
def restated(name):
    """The groups of GEOMS[name] from the Python restatement, (own, commands,
    delays) each (computed once; not to be changed)."""
    p = params(name)
    return [ft.synth_table_groups_c6(p, g) for g in range(p.groups)]


def pack(groups, n, keys):
    """pack_table_groups over generated groups, every group's lists with its
    own delays: the planes, the route plane and steps_out do not depend on the
    delays, and a group's words of targets are those of the group packed
    alone."""
    import numpy as np
    planes, route, plain, steps_out = ft.pack_table_groups([(own, cmds) for own, cmds, _ in groups], n, keys)
    parts = [ft.pack_table_groups([(own, cmds)], n, keys, delays)[2] for own, cmds, delays in groups]
    targets = np.concatenate(parts + [np.zeros(0, np.uint32)]).astype(np.uint32)
    assert np.array_equal(targets & ~np.uint32(DELAY_BITS), plain)
    return planes, route, targets, steps_out


@functools.lru_cache(maxsize=None)
def packed(name):
    p = params(name)
    return pack(restated(name), p.n, p.keys)


@functools.lru_cache(maxsize=None)
def closed(name):
    """The closed loop of every group of GEOMS[name] restated on the CPU with
    the generated delays (tests/test_table_groups_gpu.trace: streams, results,
    rounds, most_due, most_sends)."""
    from test_table_groups_gpu import trace
    p = params(name)
    return [trace(own, cmds, p.n, threshold(name), p.keys, delays) for own, cmds, delays in restated(name)]
