"""The generator of closed-loop shard groups on the device
(fx_table_group_synth_count / fx_table_group_synth_generate) against its host
twin, word for word, and fx_table_run_groups over groups that never leave the
device against the closed loop restated on the CPU.  GPU only."""
import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import table as ft

import table_group_synth_shapes as GS
from test_sim_poison import FILLS, poisoner
from test_table_groups_gpu import same

pytestmark = pytest.mark.gpu

FILL, FILL_WORD = 0xA5, 0xA5A5A5A5
PLANES = ("hdr", "dot", "clock", "votes", "nkeys")


def assert_same(dev, host):
    """Two (planes, route, targets, steps_out): every word, the lengths included."""
    (dp, droute, dtargets, dout), (hp, hroute, htargets, hout) = dev, host
    assert (dp.S, dp.steps, dp.vmax, dp.plane, dout) == (hp.S, hp.steps, hp.vmax, hp.plane, hout)
    assert np.array_equal(dp.lengths, hp.lengths)
    for name, a, b in [(name, getattr(dp, name), getattr(hp, name)) for name in PLANES] + \
            [("route", droute, hroute), ("targets", dtargets, htargets)]:
        assert a.shape == b.shape, name
        assert np.array_equal(a, b), "%s differs at word %d" % (name, int(np.flatnonzero(a != b)[0]))


@pytest.mark.parametrize("name", sorted(GS.GEOMS))
def test_device_bytes_equal_the_host_twin(gpu, name):
    """One generate per geometry over buffers filled with 0xA5 bytes: every
    word of every plane, padding included, route, targets, the lengths, and
    what the counting pass returns."""
    p = GS.params(name)
    t = fd.DeviceTableGroups(p)
    lengths, longest, steps_out, words = ft.table_group_synth_counts_host(p)
    assert (t.longest, t.steps_out, t.list_words) == (longest, steps_out, words)
    assert np.array_equal(t.lengths.download(np.uint32, t.S), lengths)
    t.fill_bytes(FILL)
    assert t.generate() == _lib.FX_OK
    assert_same(t.download(), ft.synth_table_groups_host(p))


def test_spare_rows_are_zeroed_and_spare_targets_left(gpu):
    p = GS.params("g65_p3")
    first = fd.DeviceTableGroups(p)
    t = fd.DeviceTableGroups(p, steps=first.longest + 5, targets_words=first.list_words + 3)
    t.fill_bytes(FILL)
    assert t.generate() == _lib.FX_OK
    planes, route, targets, steps_out = t.download()
    assert np.all(targets[first.list_words:] == FILL_WORD)
    host = ft.synth_table_groups_host(p, steps=first.longest + 5)
    assert_same((planes, route, targets[:first.list_words], steps_out), host)


@pytest.mark.parametrize("short", ["steps", "targets_words"])
def test_one_short_leaves_every_buffer(gpu, short):
    p = GS.params("g65_p3")
    first = fd.DeviceTableGroups(p)
    kw = dict(steps=first.longest, targets_words=first.list_words)
    kw[short] -= 1
    t = fd.DeviceTableGroups(p, **kw)
    t.fill_bytes(FILL)
    assert t.generate() == _lib.FX_ERR_CAPACITY
    planes, route, targets, _ = t.download()
    for name in PLANES:
        assert np.all(getattr(planes, name) == FILL_WORD), name
    assert np.all(route == FILL_WORD) and np.all(targets == FILL_WORD) and np.all(planes.lengths == FILL_WORD)
    with pytest.raises(_lib.FxError):
        fd.synth_table_groups(p, **kw)


def test_tiles_download_alone(gpu):
    t = fd.synth_table_groups(GS.params("g65_p3"))
    whole, route = t.download()[:2]
    for tile, first in ((0, 0), (3, 192)):
        part, part_route = t.download_tile(tile)
        for s in range(part.S):
            assert part.stream(s) == whole.stream(first + s)
            rows = np.arange(int(part.lengths[s]))
            assert np.array_equal(part_route[_lib.index(rows, s, part.steps)],
                                  route[_lib.index(rows, first + s, whole.steps)])
    assert t.download_tile(3)[0].S == 3


@pytest.mark.parametrize("name", ["g65_p3", "p8_msg31"])
def test_generate_and_execute_on_the_device(gpu, name):
    """synth_table_groups -> fx_table_run_groups with no host copy of the
    groups: the streams as handled (handled_src / handled_dot over the
    downloaded own events), order, release, stable_sent, nexec, err, the
    stable clocks and the rounds of every stream against the closed loop
    restated over the downloaded groups with the generated delays."""
    p = GS.params(name)
    t = fd.synth_table_groups(p)
    res = t.run(GS.threshold(name))
    planes = t.download()[0]
    groups = []
    for g, (own, commands, _) in enumerate(GS.restated(name)):
        assert [planes.stream(g * p.shards + h) for h in range(p.shards)] == own
        groups.append((own, commands))
    got = fd.table_group_dicts(groups, res)
    for g, want in enumerate(GS.closed(name)):
        same(got[g], want)
    assert all(r["err"] == 0 and r["nexec"] > 0 for one in got for r in one["results"])
    assert sum(ev[0] == "S" for one in got for st in one["streams"] for ev in st) > 100


@pytest.mark.parametrize("fill", FILLS, ids=["tag%02x" % t if m == 1 else "zero" for m, t in FILLS])
@pytest.mark.parametrize("name", ["onchip_p2", "scratch_p3"])
def test_poisoned_registers_do_not_change_the_groups(gpu, name, fill):
    """The register file filled with garbage (tests/poison) before the
    generator's launches, state on chip and in scratch."""
    p = GS.params(name)
    t = fd.synth_table_groups(p, before_launch=poisoner(*fill))
    assert_same(t.download(), ft.synth_table_groups_host(p))
