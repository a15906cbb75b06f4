"""fx_kv_monitor_compare_host on every edge case of monitor_edges: every pair's answer against the restatement
(monitor_ref), and the sides' buffers byte for byte as they were.  CPU only."""
import pytest

import monitor_edges as E
from fantoch_amd import kv as K


@pytest.mark.parametrize("name", E.NAMES, ids=E.IDS)
def test_host_twin_equals_the_restatement(name):
    c = E.case(name)
    before = [x.tobytes() for m in (c.a, c.b) for x in m.arrays()]
    got = K.compare_monitors_host(c.a.result(), c.a.rifl, c.b.result(), c.b.rifl, c.pairs)
    assert len(got) == len(c.want)
    for p, g, w in zip(c.pairs, got, c.want):
        assert g == w, "%s: pair %s: %s, want %s" % (name, p, g, w)
    assert before == [x.tobytes() for m in (c.a, c.b) for x in m.arrays()], name
