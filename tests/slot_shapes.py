"""The slot executor's cases: the smallest batches at which the kernels can
still go wrong, each with the planes the restatement (slot_ref) expects of a
tier, fill included.  Shared by the CPU and the GPU tests."""
import itertools

import numpy as np

from fantoch_amd import _lib
from fantoch_amd import slot as fslot

import slot_ref

LANE, SCAN = fslot.LANE, fslot.SCAN
C, SLOT = slot_ref.CAPACITY, slot_ref.SLOT
FILL = 0xA5
A5 = 0xA5A5A5A5
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 128, 129, 257)
WINDOWS = (1, 2, 8, 64)


def window_of(tier):
    """The restatement's window for a tier: the LANE tier's 64, else unbounded (SCAN, fx_slot_run, the host)."""
    return fslot.LANE_WINDOW if tier == LANE else None


class Case:
    def __init__(self, name, streams, steps=None):
        self.name, self.streams = name, streams
        self.plane, self.lengths, self.S, self.steps = fslot.pack_slot_streams(streams, steps)
        self._restated = {}

    def restated(self, s, tier, at_commit=False):
        key = (s, window_of(tier), at_commit)
        if key not in self._restated:
            self._restated[key] = slot_ref.run(self.streams[s], self.steps, window_of(tier), at_commit)
        return self._restated[key]

    def expected(self, tier, at_commit=False, only=None):
        """order, release, nexec, err as a tier must leave them over buffers of 0xA5 bytes
        (only: the streams a launch covers; the others keep the fill)."""
        pw = _lib.plane_words(self.S, self.steps)
        order, release = np.full(pw, A5, np.uint32), np.full(pw, A5, np.uint32)
        nexec, err = np.full(self.S, A5, np.uint32), np.full(self.S, A5, np.uint32)
        for s in range(self.S):
            if only is not None and s not in only:
                continue
            r = self.restated(s, tier, at_commit)
            if r["order"]:
                order[_lib.index(np.arange(r["nexec"]), s, self.steps)] = \
                    np.asarray(r["order"], np.uint32) | np.uint32(slot_ref.SCC_START)
            for a, v in r["release"].items():
                release[int(_lib.index(a, s, self.steps))] = v
            nexec[s], err[s] = r["nexec"], r["err"]
        return dict(order=order, release=release, nexec=nexec, err=err)

    def check(self, res, tier, at_commit=False, only=None):
        want = self.expected(tier, at_commit, only)
        for name in fslot.NAMES:
            a, b = getattr(res, name), want[name]
            assert np.array_equal(a, b), "%s: %s differs at word %d" % (self.name, name, int(np.flatnonzero(a != b)[0]))

    def reruns(self, at_commit=False):
        """Streams the LANE tier stops with CAPACITY: the ones fx_slot_run runs again."""
        return sum(self.restated(s, LANE, at_commit)["err"] == C for s in range(self.S))

    def run_host(self, at_commit=False):
        return fslot.run_slot_host(self.plane, self.lengths, self.S, self.steps, at_commit, fill=FILL)


def generated(L, window, seed, g):
    """One generated stream of L slots (the Python restatement of the generator)."""
    return fslot.synth_slot_streams_c6(seed, 1, L, window, stream_base=g)[0] if L else []


def flow():
    """slot_executor_flow (slot.rs:132-212): every permutation of six slots."""
    return Case("flow", [list(p) for p in itertools.permutations(range(1, 7))])


def lengths():
    streams = []
    for i, L in enumerate(LENGTHS):
        streams.append(list(range(1, L + 1)))
        streams.append(list(range(L, 0, -1)))
        streams += [generated(L, w, 11, 16 * i + w) for w in WINDOWS]
    return Case("lengths", streams)


def window_edge():
    steps = 130
    rest = lambda first: [first] + [s for s in range(1, steps + 1) if s != first]
    return Case("window edge", [rest(64), rest(65), list(range(64, 0, -1)), list(range(65, 0, -1))], steps)


def holes():
    L, streams = 40, []
    for k in (1, 20, 40):
        streams.append([s for s in generated(L, 8, 5, k) if s != k])
    return Case("holes", streams, 44)


def errors():
    steps = 80
    streams = [
        [0, 1, 2],                        # slot 0 at row 0
        [2, 1, 3, 0, 4, 5],               # slot 0 at a middle row
        [1, 2, 3, 2, 4],                  # a repeat of an executed slot
        [1, 3, 5, 3, 2, 4],               # a repeat of a waiting slot
        [1, 70, 2, 2, 3],                 # a repeat behind a row beyond the lane window
        [1, 2, 81, 3],                    # a slot above steps, beyond the lane window too
        list(range(1, 76)) + [81, 76],    # a slot above steps, within the lane window
        [1, 0, 3, 3],                     # two bad rows: the earlier one wins
        [1, 3, 3, 0],
        [2, 81, 2, 0, 1],
        [5, 4, 6, 1, 2, 2, 3],            # rows before the failing row stand, waiting ones included
    ]
    return Case("errors", streams, steps)


def batch(S):
    """S streams of mixed lengths and windows inside one tile."""
    steps = 44
    return Case("batch %d" % S, [generated((7 * s + 3) % (steps + 1), (1, 3, 8, 64)[s % 4], 7, s) for s in range(S)],
                steps)


def all_cases():
    return [flow(), lengths(), window_edge(), holes(), errors()] + [batch(S) for S in (1, 63, 64, 65, 130)]


# ------------------------------------------------------------------ the KV chain of slot_executor_flow
def flow_ops():
    """Six slots on one key, Put / Get alternating: slot s is Put(value (s + 1) / 2) for odd s, else Get."""
    from fantoch_amd import kv as K
    return {s: K.kv_op(K.PUT, (s + 1) // 2) if s % 2 else K.kv_op(K.GET) for s in range(1, 7)}
