"""Geometries of the seeded Tempo stream generator (fx_table_synth_*) shared by
tests/test_table_synth_cpu.py and tests/test_table_synth_gpu.py: keyword
arguments of fantoch_amd.table.table_synth_params.  Together they cover
S = 1 and S = 65 (a second tile of one stream), (n, fast quorum) = (3, 2),
(5, 3), (7, 4), (16, 9), keys = 1, 2 (with kmax = 2 the key pick exhausts the
pool), 16, 33 and 64, kmax = 1, 2, 3, conflict rates 0, 2, 100 and two rates
split by conflict_block, (window, lag) = (0, 0), (4, 6), (50, 80), (9, 3), and
cmds = 0 and 1.  Per-stream state is (keys + 1) * n words: on chip up to
FX_TABLE_SYNTH_ONCHIP_WORDS = 256 (keys33_n5: 170), in scratch above
(keys64_n5: 325, n16: 544)."""
import functools

from fantoch_amd import table as ft

GEOMS = {
    "s1_n3_keys1": dict(streams=1, n=3, fast_quorum=2, keys=1, kmax=1, cmds=40, conflicts=(0,), window=0, lag=0),
    "s65_n5_k2": dict(streams=65, n=5, fast_quorum=3, keys=16, kmax=2, cmds=40, conflicts=(2, 50), conflict_block=32,
                      window=4, lag=6),
    "s65_n5_k1_late": dict(streams=65, n=5, fast_quorum=3, keys=16, kmax=1, cmds=37, conflicts=(2,), window=50, lag=80),
    "n7_keys2_k2": dict(streams=3, n=7, fast_quorum=4, keys=2, kmax=2, cmds=60, conflicts=(100,), window=9, lag=3),
    "n16_keys33_k3": dict(streams=2, n=16, fast_quorum=9, keys=33, kmax=3, cmds=30, conflicts=(2,), window=50, lag=80),
    "keys33_n5": dict(streams=5, n=5, fast_quorum=3, keys=33, kmax=3, cmds=40, conflicts=(0, 100), window=4, lag=6),
    "keys64_n5": dict(streams=66, n=5, fast_quorum=3, keys=64, kmax=3, cmds=25, conflicts=(2,), window=4, lag=6),
    "keys1_k3": dict(streams=3, n=5, fast_quorum=3, keys=1, kmax=3, cmds=30, conflicts=(2,), window=9, lag=3),
    "cmds0": dict(streams=3, n=5, fast_quorum=3, keys=16, kmax=2, cmds=0, conflicts=(2,), window=4, lag=6),
    "cmds1": dict(streams=3, n=5, fast_quorum=5, keys=16, kmax=2, cmds=1, conflicts=(2,), window=4, lag=6),
}
SEED, BASE = 20240607, 1000


def params(name, **over):
    kw = dict(GEOMS[name], seed=SEED, stream_base=BASE)
    kw.update(over)
    return ft.table_synth_params(**kw)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The streams of GEOMS[name] from the Python restatement (computed once; not to be changed)."""
    p = params(name)
    return [ft.synth_table_streams_c6(p, s) for s in range(p.streams)]
