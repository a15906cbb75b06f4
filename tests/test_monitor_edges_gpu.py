"""fx_kv_monitor_compare (k_kv_compare) on every edge case of monitor_edges: every pair's answer against the host
twin and against the restatement (monitor_ref); the words of `diff` behind the last pair and every buffer of both
sides byte for byte as they were; the register file filled with garbage before every launch.  Then monitors that
executors wrote: a session fed in pieces against fx_kv_execute, and one seeded disagreement.  Each side's
buffers go to the device once.  GPU only."""
import functools
import random

import numpy as np
import pytest

import kv_shapes as KS
import monitor_edges as E
import monitor_ref as M
from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import kv as K
from test_sim_poison import FILLS, poisoner

pytestmark = pytest.mark.gpu
PAD = 7  # words of `diff` behind the last pair


@functools.lru_cache(maxsize=None)
def on_device(side):
    """The side's buffers on the device (sides are kept by identity: monitor_edges builds each once)."""
    keep = []
    return {name: fd._dev(x, keep) for name, x in zip(("monitor", "mon_off", "rifl"), side.arrays())}


def device_bytes(side):
    return [buf.download(np.uint32, x.size).tobytes() for buf, x in zip(on_device(side).values(), side.arrays())]


@pytest.mark.parametrize("i", range(len(E.NAMES)), ids=E.IDS)
def test_device_equals_the_host_twin_and_the_restatement(gpu, i):
    c = E.all_cases()[i]
    da, db = on_device(c.a), on_device(c.b)
    got, pad = fd.compare_monitors(c.a.result(da), da["rifl"], c.b.result(db), db["rifl"], c.pairs,
                                   before_launch=poisoner(*FILLS[i % len(FILLS)]), diff_pad=PAD)
    host = K.compare_monitors_host(c.a.result(), c.a.rifl, c.b.result(), c.b.rifl, c.pairs)
    assert len(got) == len(c.pairs)
    for p, g, h, w in zip(c.pairs, got, host, c.want):
        assert g == h == w, "%s: pair %s: device %s, host twin %s, restatement %s" % (c.name, p, g, h, w)
    assert len(pad) == PAD and np.all(pad == E.A5), c.name
    for m in (c.a, c.b):
        assert device_bytes(m) == [x.tobytes() for x in m.arrays()], c.name


@pytest.mark.parametrize("fill", FILLS, ids=str)
def test_every_fill_of_the_register_file(gpu, fill):
    for name in ("key strips, 600 keys", "row chunks, 129 rows", "pairs that cannot be compared, sides swapped"):
        c = E.case(name)
        da, db = on_device(c.a), on_device(c.b)
        got = fd.compare_monitors(c.a.result(da), da["rifl"], c.b.result(db), db["rifl"], c.pairs,
                                  before_launch=poisoner(*fill))
        assert got == c.want, name


# ------------------------------------------------------------------ monitors that executors wrote
ROWS, SWAP_AT = 150, 80  # order rows SWAP_AT and SWAP_AT + 1 of stream 1 are swapped: beyond order row 64


def chain_case(swap=False):
    """3 streams of 150 rows on ABOVE keys, executed in the reverse of their arrival; order rows 80 and 81 of every
    stream are writes of the last key, which has more of them before and behind."""
    rng = random.Random(17)
    hot = E.ABOVE - 1
    sts = []
    for s in range(3):
        order = list(range(ROWS - 1, -1, -1))
        keys_of = [rng.choice([hot, hot, 7, 64, 65, 300, rng.randrange(E.ABOVE)]) for _ in range(ROWS)]
        ops_of = [[KS.G] if a % 5 == 0 else [KS.D] if a % 7 == 0 else [KS.P(1 + a)] for a in range(ROWS)]
        for k in (SWAP_AT, SWAP_AT + 1):
            keys_of[order[k]], ops_of[order[k]] = hot, [KS.P(9000 + k)]
        if swap and s == 1:
            order[SWAP_AT], order[SWAP_AT + 1] = order[SWAP_AT + 1], order[SWAP_AT]
        sts.append(KS.stream(order, keys_of, ops_of))
    case = KS.Case("chain", sts, E.ABOVE, 1)
    rifl = np.full(case.plane, E.A5, np.uint32)
    for s in range(3):
        rifl[_lib.index(np.arange(ROWS), s, ROWS)] = 0x20000 + 1000 * s + np.arange(ROWS)
    return case, rifl


def run_whole(case):
    return fd.run_kv(case.order, case.nexec, case.key, case.ops, case.S, case.steps, case.keys, case.omax, case.key_mask,
                     fill=0xA5, before_launch=poisoner(*FILLS[0]), keep_device=True)


def test_a_session_in_pieces_agrees_with_one_execution_and_a_swap_is_found(gpu):
    case, rifl = chain_case()
    assert (case.S, case.steps, case.keys) == (3, ROWS, _lib.FX_KV_ONCHIP_KEYS + 88)
    whole = run_whole(case)
    assert np.all(whole.err == 0)
    ses = K.KvSession(case.S, case.steps, case.keys, case.omax, fill=0xA5)
    done = 0
    for piece in (63, 64, 23):
        done += piece
        res = ses.advance(case.order, np.full(case.S, done, np.uint32), case.key, case.ops, case.key_mask,
                          before_launch=poisoner(*FILLS[1]))
        assert np.all(res.err == 0)
    assert done == ROWS
    mon = ses.monitor(fill=0xA5, before_launch=poisoner(*FILLS[1]))
    same = [(s, s) for s in range(case.S)]
    got = fd.compare_monitors(mon, rifl, whole, rifl, same, before_launch=poisoner(*FILLS[2]))
    assert got == [M.AGREE] * case.S == [M.compare(E.View(mon, rifl), s, E.View(whole, rifl), s) for s in range(case.S)]
    assert int(whole.mon_off[1, case.keys]) > 64  # more than one chunk of monitor rows
    # stream 1 with two adjacent writes of one key the other way round
    other, _ = chain_case(swap=True)
    swapped = run_whole(other)
    want = [M.compare(E.View(mon, rifl), s, E.View(swapped, rifl), s) for s in range(case.S)]
    hot = case.keys - 1
    before = sum(1 for k in range(SWAP_AT) if case.streams[1]["keys_of"][case.streams[1]["order"][k]] == hot and
                 case.streams[1]["ops_of"][case.streams[1]["order"][k]] != [KS.G])
    assert want == [M.AGREE, (hot, before), M.AGREE] and before >= 1
    assert int(whole.mon_off[1, hot]) + before >= 64  # the differing monitor row lies in a later chunk
    assert fd.compare_monitors(mon, rifl, swapped, rifl, same, before_launch=poisoner(*FILLS[0])) == want
    assert fd.compare_monitors(swapped, rifl, mon, rifl, same) == want
    assert K.compare_monitors_host(mon, rifl, swapped, rifl, same) == want
