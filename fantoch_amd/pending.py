"""The pending stage (fx_pending_aggregate and friends): AggregatePending for
the batched engines.  A command's partials, one order row per (rifl, key), are
collected per rifl; a command is named by its head row (the arrival row of its
first executed partial) and is ready when its last partial has executed.  The
device calls are in fantoch_amd.device (run_pending).

Canonical C16: the partials of a command are listed in execution order."""
import ctypes

import numpy as np

from . import _lib

MAX_PARTS, IGNORED = _lib.FX_PENDING_MAX_PARTS, _lib.FX_PENDING_IGNORED
ONCHIP, HBM = _lib.FX_PENDING_TIER_ONCHIP, _lib.FX_PENDING_TIER_HBM
NAMES = ("part", "head", "ready", "index", "nready", "nopen", "err")


class PendingResult:
    """Outputs of the pending stage as host arrays: part (MAX_PARTS planes by
    head row), head (plane by arrival row), ready (plane), index (plane by head
    row), nready / nopen / err [S], the call's status and the streams rerun on
    the HBM tier.  `dev` (run_pending(keep_device=True)): the device buffers by
    the same names."""

    def __init__(self, S, steps, part, head, ready, index, nready, nopen, err, status, reruns=0, dev=None):
        self.S, self.steps, self.plane = S, steps, _lib.plane_words(S, steps)
        self.part, self.head, self.ready, self.index = part, head, ready, index
        self.nready, self.nopen, self.err, self.status, self.reruns, self.dev = nready, nopen, err, status, reruns, dev
        # the rifl and count planes the call read with its count_mask and process (host copies):
        # command_results names a command and counts its partials with them
        self.rifl = self.count = None
        self.count_mask, self.process = 0xFFFFFFFF, 0

    def members(self, s, head):
        """The partials of the command with head row `head`: the count the stage read at that row."""
        at = int(_lib.index(head, s, self.steps))
        if self.process and int(self.rifl[at]) >> 24 != self.process:
            return 0
        return int(self.count[at]) & self.count_mask

    def ready_heads(self, s):
        """Head rows of the completed commands of stream s, in completion order."""
        return [int(h) for h in self.ready[_lib.index(np.arange(int(self.nready[s])), s, self.steps)]]

    def parts(self, s, head, count):
        """Arrival rows of the first `count` partials of the command with head row `head`."""
        at = int(_lib.index(head, s, self.steps))
        return [int(self.part[j * self.plane + at]) for j in range(count)]


def _u32(a):
    return np.ascontiguousarray(a, np.uint32)


def run_pending_host(order, nexec, rifl, count, S, steps, count_mask=0xFFFFFFFF, process=0, tier=HBM, fill=0):
    """fx_pending_aggregate_host over host arrays; every output starts filled
    with the byte `fill`.  Returns a PendingResult (a refused call: its status,
    outputs as filled)."""
    order, nexec, rifl, count = _u32(order), _u32(nexec), _u32(rifl), _u32(count)
    pw = _lib.plane_words(S, steps)
    word = np.uint32(fill * 0x01010101)
    out = {name: np.full(n, word, np.uint32)
           for name, n in zip(NAMES, (MAX_PARTS * pw, pw, pw, pw, S, S, S))}
    inb = _lib.PendingBatch(order.ctypes.data, nexec.ctypes.data, rifl.ctypes.data, count.ctypes.data, count_mask,
                            process, S, steps)
    outb = _lib.PendingOut(*[out[name].ctypes.data for name in NAMES])
    status = _lib.load().fx_pending_aggregate_host(ctypes.byref(inb), ctypes.byref(outb), tier)
    res = PendingResult(S, steps, *[out[name] for name in NAMES], status)
    res.rifl, res.count, res.count_mask, res.process = rifl, count, count_mask, process
    return res


def command_results(pending, kv, key_plane, s, key_mask=0xFFFFFFFF, ops=None):
    """The CommandResults of stream s, in completion order: [(rifl, {key:
    [results]})], a result None or the value's id.  pending: a PendingResult;
    kv: the KvResult of the same order plane; key_plane: the key plane the KV
    stage read.  A command's rifl and the number of its partials are the rifl
    and the count the pending stage read at its head row (a completed command
    has exactly that many), so nothing here depends on what the outputs held
    before the call.  ops (the op planes): a partial's results stop at its
    first unused slot; without them every partial has kv.omax."""
    steps, rifl = pending.steps, pending.rifl
    out = []
    for h in pending.ready_heads(s):
        per_key = {}
        for a in pending.parts(s, h, pending.members(s, h)):
            at = int(_lib.index(a, s, steps))
            res = kv.results(s, a)
            if ops is not None:
                res = [r for j, r in enumerate(res) if int(ops[j * pending.plane + at]) >> 30 != _lib.FX_KV_EMPTY]
            per_key[int(key_plane[at]) & key_mask] = [r or None for r in res]
        out.append((int(rifl[int(_lib.index(h, s, steps))]), per_key))
    return out
