"""Shared inputs of the table-executor tests: the reference's known-answer
tests (tests/golden/table_kat.json) as event streams, the generated Tempo
streams, and the restatement's results computed once per case."""
import functools
import itertools
import json
import os

from fantoch_amd import table as ft

import table_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = json.load(open(os.path.join(HERE, "golden", "table_kat.json")))

# (n, f, tiny quorums) of the generated streams; conflict rates; sizes
CONFIGS = [(3, 1, False), (5, 1, True), (5, 2, False), (5, 2, True), (7, 3, False)]
CONFLICTS = [0, 10, 100]
SEEDS, KEYS, CMDS, LAG, WINDOW = 24, 8, 40, 6, 4


def quorum_sizes(n, f, tiny):
    """Config::tempo_quorum_sizes (fantoch/src/config.rs:337-349) restated, so
    the CPU tests of the generator need no library."""
    minority = n // 2
    return (2 * f, f + 1, n - f) if tiny else (minority + f, f + 1, minority + 1)


def kat_event(case, name, key=0):
    op = KAT[case]["ops"][name]
    return ("A", key, tuple(op["dot"]), op["clock"], [tuple(v) for v in op["votes"]])


def kat_stream(case, names):
    return [kat_event(case, nm) for nm in names]


def majority_streams():
    """The 120 permutations of the five ops, then the stepwise sequence."""
    names = sorted(KAT["majority"]["ops"])
    return [list(p) for p in itertools.permutations(names)] + [list(KAT["majority"]["stepwise"])]


def detached_events():
    d = KAT["detached"]
    return [("D", d["keys"].index(k), [tuple(v)]) for k, v in d["events"]]


@functools.lru_cache(maxsize=None)
def generated(n, f, tiny, conflict, count=SEEDS, cmds=CMDS, lag=LAG, window=WINDOW, keys=KEYS):
    """`count` generated streams (seeds 0..count-1) of one configuration."""
    fq = quorum_sizes(n, f, tiny)[0]
    return tuple(tuple(ft.synth_table_streams(1000 * conflict + seed, n, fq, keys, cmds, conflict, lag, window))
                 for seed in range(count))


@functools.lru_cache(maxsize=None)
def generated_ref(n, f, tiny, conflict, count=SEEDS, cmds=CMDS, lag=LAG, window=WINDOW, keys=KEYS):
    thr = quorum_sizes(n, f, tiny)[2]
    return tuple(R.run_stream(list(st), n, thr, keys)
                 for st in generated(n, f, tiny, conflict, count, cmds, lag, window, keys))
