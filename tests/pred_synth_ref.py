"""The Caesar commit-stream model (csrc/fx_pred_synth.h)
restated in plain Python integers, independently of the library: the counter
RNG, keys, retries, clocks, deps, delivery, and the planes a generator must
leave on buffers pre-filled with a poison word (test infrastructure)."""
from collections import namedtuple

import numpy as np

M64 = (1 << 64) - 1
PURPOSE_KEY, PURPOSE_JITTER, PURPOSE_RETRY = 1, 3, 5
POISON = 0xA5A5A5A5

Params = namedtuple("Params", "seed instances instance_base n cmds window horizon max_bump retry_pct conflicts "
                              "conflict_block")


def params(seed=1, instances=1, n=5, cmds=100, window=8, horizon=4, max_bump=2, retry_pct=30,
           conflicts=(2, 10, 50, 100), instance_base=0, conflict_block=0):
    return Params(seed, instances, instance_base, n, cmds, window, horizon, max_bump, retry_pct, tuple(conflicts),
                  conflict_block)


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def rand(seed, inst, a, b):
    return mix64((mix64((mix64(seed ^ 0x5851F42D4C957F2D) + inst) & M64) + (a << 8) + b) & M64)


def shape(p):
    return p.instances * p.n, p.n * p.cmds, p.n * (p.horizon + p.max_bump + 1) - 1


def plane_words(S, steps):
    return (S + 63) // 64 * 64 * ((steps + 3) // 4) * 4


def index(step, stream, steps):
    return ((stream >> 6) * ((steps + 3) >> 2) + (step >> 2)) * 256 + ((stream & 63) << 2) + (step & 3)


class Instance:
    """One instance: per command g its key, bump, clocks and deps; per process its delivery order."""

    def __init__(self, p, local):
        self.p, self.inst = p, p.instance_base + local
        n, N = p.n, p.n * p.cmds
        nc = len(p.conflicts) or 1
        ci = (self.inst // p.conflict_block) % nc if p.conflict_block else self.inst % nc
        self.rate = p.conflicts[ci] if p.conflicts else 0
        K = p.max_bump + 1
        self.shared = [self._shared(g) for g in range(N)]
        self.key = [0 if self.shared[g] else g % n + 1 for g in range(N)]
        self.bump = [self._bump(g) for g in range(N)]
        self.round = [g // n + 1 for g in range(N)]
        self.source = [g % n + 1 for g in range(N)]
        self.proposal = [(K * self.round[g], self.source[g]) for g in range(N)]
        self.final = [(K * (self.round[g] + self.bump[g]) + self.bump[g], self.source[g]) for g in range(N)]
        self.deps = [self._deps(g) for g in range(N)]

    def _shared(self, g):
        if self.rate == 0:
            return False
        if self.rate >= 100:
            return True
        return rand(self.p.seed, self.inst, g, PURPOSE_KEY) % 100 < self.rate

    def _bump(self, g):
        p = self.p
        if not self.shared[g] or p.max_bump == 0:
            return 0
        x = rand(p.seed, self.inst, g, PURPOSE_RETRY)
        if x % 100 >= p.retry_pct:
            return 0
        return min(1 + (x >> 32) % p.max_bump, p.cmds - (g // p.n + 1))

    def _deps(self, g):
        """Commands g2, ascending by dot (source, round)."""
        p, j = self.p, self.round[g]
        out = [g2 for g2 in range(p.n * p.cmds)
               if g2 != g and self.key[g2] == self.key[g] and self.round[g2] >= max(1, j - p.horizon)
               and self.proposal[g2] < self.final[g]]
        return sorted(out, key=lambda g2: (self.source[g2], self.round[g2]))

    def arrival(self, proc, g):
        w = self.p.window
        if w == 0:
            return g
        return g + rand(self.p.seed, self.inst, (g << 4) | proc, PURPOSE_JITTER) % (w + 1)

    def delivery(self, proc):
        """Commands in the order process `proc` handles them: by (arrival key, g)."""
        N = self.p.n * self.p.cmds
        return sorted(range(N), key=lambda g: (self.arrival(proc, g), g))

    def dot(self, g):
        return (self.source[g] << 24) | self.round[g]


def generate(p, ndeps=True, poison=POISON):
    """The six planes (ndeps None without one) on buffers of `poison` words."""
    S, steps, dmax = shape(p)
    pw = plane_words(S, steps)
    dot, hdr, clo, chi = (np.full(pw, poison, np.uint32) for _ in range(4))
    deps = np.full(max(dmax, 1) * pw, poison, np.uint32)
    nd = np.full(pw, poison, np.uint32) if ndeps else None
    for local in range(p.instances):
        inst = Instance(p, local)
        for proc in range(1, p.n + 1):
            stream = local * p.n + proc - 1
            for rank, g in enumerate(inst.delivery(proc)):
                at = index(rank, stream, steps)
                ds = inst.deps[g]
                clock = (inst.final[g][0] << 8) | inst.final[g][1]
                dot[at] = inst.dot(g)
                hdr[at] = (inst.arrival(proc, g) & 0xFFFFFF) | (min(len(ds), 31) << 24)
                clo[at] = clock & 0xFFFFFFFF
                chi[at] = clock >> 32
                if ndeps:
                    nd[at] = len(ds)
                for k in range(dmax):
                    deps[k * pw + at] = inst.dot(ds[k]) if k < len(ds) else 0
    return dot, hdr, deps, clo, chi, nd


def dep_kinds(p):
    """(commit-only deps, execute-first deps, retried commands with a dep of a
    larger dot seq) over every instance."""
    commit_only = execute_first = later = 0
    for local in range(p.instances):
        inst = Instance(p, local)
        for g, ds in enumerate(inst.deps):
            for d in ds:
                if inst.final[d] > inst.final[g]:
                    commit_only += 1
                else:
                    execute_first += 1
            if inst.bump[g] and any(inst.round[d] > inst.round[g] for d in ds):
                later += 1
    return commit_only, execute_first, later
