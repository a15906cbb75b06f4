"""The Tempo stream generator on the device (fx_table_synth_lengths /
fx_table_synth_generate) against its host twin, word for word, and the table
executor over streams that never leave the device against the CPU
restatement.  GPU only."""
import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import table as ft

import table_ref as R
import table_ref_mk as RM
import table_synth_shapes as TS
from test_sim_poison import FILLS, poisoner
from test_table_mk_gpu import ORDER_TAG, compare

pytestmark = pytest.mark.gpu

FILL, FILL_WORD = 0xA5, 0xA5A5A5A5
PLANES = ("hdr", "dot", "clock", "votes", "nkeys")
# three tiles, the last one ragged
GEOMS = dict(TS.GEOMS, s130=dict(streams=130, n=5, fast_quorum=3, keys=16, kmax=2, cmds=40, conflicts=(2, 50),
                                 window=4, lag=6))


def make_params(name, **over):
    kw = dict(GEOMS[name], seed=TS.SEED, stream_base=TS.BASE)
    kw.update(over)
    return ft.table_synth_params(**kw)


def assert_same_planes(dev, host):
    assert (dev.S, dev.steps, dev.vmax, dev.plane) == (host.S, host.steps, host.vmax, host.plane)
    assert np.array_equal(dev.lengths, host.lengths)
    for name in PLANES:
        a, b = getattr(dev, name), getattr(host, name)
        assert (a is None) == (b is None), name
        if a is not None:
            assert np.array_equal(a, b), "%s plane differs at word %d" % (name, int(np.flatnonzero(a != b)[0]))


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_device_planes_equal_the_host_twin(gpu, name):
    """One launch per geometry over planes filled with 0xA5 bytes: every word
    of every plane, padding included, and the lengths."""
    p = make_params(name)
    t = fd.DeviceTable(p)
    host = ft.synth_table_host(p)
    assert t.longest == max(host.lengths.tolist() + [0]) and t.steps == host.steps
    t.fill_bytes(FILL)
    assert t.generate() == _lib.FX_OK
    assert_same_planes(t.download(), host)


def test_spare_rows_are_zeroed(gpu):
    p = make_params("s65_n5_k2")
    longest = fd.DeviceTable(p).longest
    t = fd.DeviceTable(p, steps=longest + 5)
    t.fill_bytes(FILL)
    assert t.generate() == _lib.FX_OK
    assert_same_planes(t.download(), ft.synth_table_host(p, steps=longest + 5))


def test_steps_too_small_leaves_the_planes(gpu):
    p = make_params("s65_n5_k2")
    longest = fd.DeviceTable(p).longest
    t = fd.DeviceTable(p, steps=longest - 1)
    t.fill_bytes(FILL)
    assert t.generate() == _lib.FX_ERR_CAPACITY
    got = t.download()
    for name in PLANES:
        assert np.all(getattr(got, name) == FILL_WORD), name
    with pytest.raises(_lib.FxError):
        fd.synth_table(p, steps=longest - 1)


def test_tiles_download_alone(gpu):
    t = fd.synth_table(make_params("s130"))
    whole = t.download()
    for tile, first in ((0, 0), (2, 128)):
        part = t.download_tile(tile)
        for s in range(part.S):
            assert part.stream(s) == whole.stream(first + s)
    assert t.download_tile(2).S == 2


@pytest.mark.parametrize("kmax,window,lag", [(1, 4, 6), (2, 4, 6), (1, 50, 80), (2, 50, 80)])
def test_generate_and_execute_on_the_device(gpu, kmax, window, lag):
    """synth_table -> run_table with no host copy of the streams: fx_table_run
    (kmax 1) and fx_table_run_mk (kmax 2) over 65 streams; order, release,
    nexec, err and the stable clocks of every stream against the restatement
    of the downloaded streams.  With commits up to 50 and detached votes up
    to 80 commands late, every other stream has all its 40 commands on key
    0: its votes reach clock 40 while frontiers still stand at 0, beyond
    FX_TABLE_ONCHIP_WINDOW = 32 (the restatement's max_above says which
    streams), so those streams rerun on the HBM tier."""
    n, keys, thr = 5, 16, 3
    p = ft.table_synth_params(seed=5, streams=65, n=n, fast_quorum=3, keys=keys, cmds=40, kmax=kmax,
                              conflicts=(2, 100) if lag == 80 else (2, 50), window=window, lag=lag)
    t = fd.synth_table(p)
    assert (t.nkeys is not None) == (kmax > 1)
    res = fd.run_table(t, thr, order_fill=ORDER_TAG)
    planes = t.download()
    ref = R if kmax == 1 else RM
    refs = []
    for s in range(65):
        st = planes.stream(s)
        assert st == ft.synth_table_streams_c6(p, s)
        refs.append(ref.run_stream(st, n, thr, keys))
    assert res.status == 0
    assert compare(planes, res, refs) == 65
    if lag == 80:
        assert any(r["max_above"] > _lib.FX_TABLE_ONCHIP_WINDOW for r in refs)
        assert res.reruns > 0


@pytest.mark.parametrize("fill", FILLS, ids=["tag%02x" % t if m == 1 else "zero" for m, t in FILLS])
@pytest.mark.parametrize("name", ["s65_n5_k2", "keys64_n5"])
def test_poisoned_registers_do_not_change_the_streams(gpu, name, fill):
    """The register file filled with garbage (tests/poison) before the
    generator's launches, state on chip and in scratch."""
    p = make_params(name)
    t = fd.synth_table(p, before_launch=poisoner(*fill))
    assert_same_planes(t.download(), ft.synth_table_host(p))
