"""The chain executor session -> fx_kv_advance -> fx_pending_advance, a piece
in and that piece's results, stores and completed commands out: after every
piece the stage sessions equal fx_kv_execute / fx_pending_run over the
executor session's device-resident order plane with that piece's nexec, and
after the last piece the bytes of the whole chain.  GPU only."""
import copy

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd import device as fd
from fantoch_amd import kv as K
from fantoch_amd import pending as P
from fantoch_amd import slot as fslot
from fantoch_amd import table as ft

import kv_resume as KR
import kv_shapes as KS
import pending_resume as PR
from test_sim_poison import FILLS, poisoner

pytestmark = pytest.mark.gpu

FILL = 0xA5
KV_FIELDS = ("result", "store", "monitor", "mon_off", "err")


def stages_equal(kvs, pend, kv_whole, pend_whole, what):
    """The two sessions against the whole stages over the same order plane and nexec."""
    got = kvs.result()
    KR.same("the KV session", got, kv_whole, what, ("result", "store", "err"))
    KR.same("the KV session's monitor", kvs.monitor(fill=FILL), kv_whole, what, KV_FIELDS)
    PR.same("the pending session", pend.result(), pend_whole, what)
    return got


def test_generated_slot_streams_in_four_pieces(gpu):
    """fx_slot_synth_generate -> four fx_slot_advance, each followed by fx_kv_advance and fx_pending_advance.
    Slots 2k - 1 and 2k are the two partials of command k, so commands straddle the pieces."""
    S, steps, window, keys = 65, 200, 100, 16
    plane = fslot.synth_slot(9, S, steps, window, fill=FILL, before_launch=poisoner(*FILLS[0]))
    ops = fd.synth_kv_ops(6, S, steps, read_pct=40, delete_pct=10)
    pw = _lib.plane_words(S, steps)
    rifl = (plane.download(np.uint32, pw) + 1) // 2
    count = np.full(pw, 2, np.uint32)
    keep = []
    rifl_d, count_d = fd._dev(rifl, keep), fd._dev(count, keep)
    ses = fslot.SlotSession(S, steps, fill=FILL)
    kvs = K.KvSession(S, steps, keys, 1, fill=FILL)
    pend = P.PendingSession(S, steps, fill=FILL)
    lengths = fd.DeviceBuffer(S * 4)
    completed, straddling = np.zeros(S, np.int64), []
    for piece in range(4):
        lens = np.array([min(steps, 50 * (piece + 1) + s % 7) if piece < 3 else steps for s in range(S)], np.uint32)
        lengths.upload(lens)
        ses.launch(plane, lengths, before_launch=poisoner(*FILLS[piece % len(FILLS)]))
        got = ses.dev
        kvs.launch(got["order"], got["nexec"], plane, ops, key_mask=keys - 1, before_launch=poisoner(*FILLS[1]))
        pend.launch(got["order"], got["nexec"], rifl_d, count_d, before_launch=poisoner(*FILLS[2]))
        kv_whole = fd.run_kv(got["order"], got["nexec"], plane, ops, S, steps, keys, 1, key_mask=keys - 1, fill=FILL)
        pend_whole = fd.run_pending(got["order"], got["nexec"], rifl_d, count_d, S, steps, fill=FILL)
        assert np.all(kv_whole.err == 0) and np.all(pend_whole.err == 0)
        stages_equal(kvs, pend, kv_whole, pend_whole, "piece %d" % piece)
        for s in (0, 33, 64):
            new = pend.new_ready(s)
            assert new == pend_whole.ready_heads(s)[int(completed[s]):]
        completed = pend_whole.nready.astype(np.int64)
        straddling.append(int(pend_whole.nopen.sum()))
    assert min(straddling[:3]) > 20 and straddling[3] == 0  # builders live across every cut
    assert np.all(completed == steps // 2) and np.all(pend.result().nopen == 0)
    # the bytes of the whole chain
    whole = fslot.run_slot(plane, None, S, steps, fill=FILL, keep_device=True)
    assert np.all(whole.err == 0) and np.all(whole.nexec == steps)
    stages_equal(kvs, pend,
                 fd.run_kv(whole.dev["order"], whole.dev["nexec"], plane, ops, S, steps, keys, 1, key_mask=keys - 1,
                           fill=FILL),
                 fd.run_pending(whole.dev["order"], whole.dev["nexec"], rifl_d, count_d, S, steps, fill=FILL),
                 "the whole chain")


def test_table_streams_in_three_pieces_and_their_command_results(gpu):
    """kv_shapes.table_batch(mk=True), commands of up to 2 partials, behind fx_table_advance in 3 pieces.
    command_results over new_ready of every piece, concatenated, equals command_results of the whole run.  (Whether
    a builder is live at a cut is up to the executor's order; the slot chain above has them at every cut.)"""
    batch = KS.table_batch(True)
    KS.check_precondition(batch)
    planes = ft.pack_table_streams([b[0] for b in batch], KS.N, KS.KEYS)
    ops, omax = K.pack_kv_ops([b[3] for b in batch], planes.steps, omax=2)
    S, steps = planes.S, planes.steps
    full = np.asarray(planes.lengths, np.uint32) if planes.lengths is not None else np.full(S, steps, np.uint32)
    keep = []
    ops_d = fd._dev(ops, keep)
    tab = fd.TableSession(S, steps, planes.n, planes.keys, planes.vmax, KS.THR, _lib.FX_TABLE_KIND_MK, order_fill=FILL)
    kvs = K.KvSession(S, steps, KS.KEYS, omax, fill=FILL)
    pend = P.PendingSession(S, steps, fill=FILL)
    pieces = [[] for _ in range(S)]
    for piece in range(3):
        p = copy.copy(planes)
        p.lengths = np.array([min(int(L), (int(L) * (piece + 1)) // 3 + s % 5) if piece < 2 else int(L)
                              for s, L in enumerate(full)], np.uint32)
        tab.advance(p)
        kvs.launch(tab.order, tab.nexec, tab.bufs["hdr"], ops_d, key_mask=0x00FFFFFF,
                   before_launch=poisoner(*FILLS[piece % len(FILLS)]))
        pend.launch(tab.order, tab.nexec, tab.bufs["dot"], tab.nkeys, before_launch=poisoner(*FILLS[1]))
        kv_whole = fd.run_kv(tab.order, tab.nexec, tab.bufs["hdr"], ops_d, S, steps, KS.KEYS, omax,
                             key_mask=0x00FFFFFF, fill=FILL)
        pend_whole = fd.run_pending(tab.order, tab.nexec, tab.bufs["dot"], tab.nkeys, S, steps, fill=FILL)
        assert np.all(kv_whole.err == 0) and np.all(pend_whole.err == 0)
        kv_now = stages_equal(kvs, pend, kv_whole, pend_whole, "piece %d" % piece)
        res = pend.result()
        for s in range(S):
            sofar = P.command_results(res, kv_now, planes.hdr, s, key_mask=0x00FFFFFF, ops=ops)
            new = pend.new_ready(s)
            assert new == res.ready_heads(s)[len(pieces[s]):]
            pieces[s] += sofar[len(pieces[s]):]
    assert np.all(pend.result().nopen == 0)
    whole = fd.run_table(planes, KS.THR, keep_device=True, order_fill=FILL)
    assert np.all(whole.err == 0)
    kv_whole = fd.run_kv(whole.dev["order"], whole.dev["nexec"], whole.dev["hdr"], ops_d, S, steps, KS.KEYS, omax,
                         key_mask=0x00FFFFFF, fill=FILL)
    nkeys = fd._dev(planes.nkeys, keep)
    pend_whole = fd.run_pending(whole.dev["order"], whole.dev["nexec"], whole.dev["dot"], nkeys, S, steps, fill=FILL)
    stages_equal(kvs, pend, kv_whole, pend_whole, "the whole chain")
    for s in range(S):
        want = P.command_results(pend_whole, kv_whole, planes.hdr, s, key_mask=0x00FFFFFF, ops=ops)
        assert pieces[s] == want and len(want) > 0
