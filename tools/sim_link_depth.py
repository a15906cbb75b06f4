"""Messages in flight on one process link, from the FX_SIM_PROFILE build (make
prof): stat 31 of an instance is the most any of its process links held at
once.  Over the configs[1] mix (EPaxos n = 5) per conflict rate, configs[0]
(Atlas n = 3) over the same rates, over every --stride'th
placement of configs[2] (Atlas n = 5 / 7, every region subset), and with --far
over a synthetic planet whose third process region moves away in 10 ms steps
(the sweep the pinned cases of tests/test_sim_link_lanes.py come from).  First
launch only (tiered=False).  A build that keeps the links in lanes stops an
instance at its depth D, so the distribution is taken from a pool build:
--generic, or a library built with -DFX_LINK_D=0.

usage: FX_LIB=fantoch_amd/build_prof/libfantoch_amd.so python tools/sim_link_depth.py [--seeds N] [--cmds M]
       [--stride K] [--generic] [--far]"""
import argparse
import itertools
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from fantoch_amd import sim as S

ap = argparse.ArgumentParser()
ap.add_argument("--seeds", type=int, default=256)
ap.add_argument("--cmds", type=int, default=1000)
ap.add_argument("--stride", type=int, default=16)
ap.add_argument("--generic", action="store_true")
ap.add_argument("--far", action="store_true")
a = ap.parse_args()
assert os.environ.get("FX_LIB"), "set FX_LIB to the profile build"
pl = S.Planet()


def report(tag, specs, planet=pl, each=False):
    res = S.run(specs, planet, lat_cap=0, tiered=False, generic=a.generic)
    depth = res.stats[:, 31].astype(np.int64)
    hist = np.bincount(depth)
    print("%-30s %6d instances, errors %d, deepest link: max %d, histogram %s"
          % (tag, len(specs), int((res.err != 0).sum()), int(depth.max()), {i: int(c) for i, c in enumerate(hist) if c}))
    if each:
        print("    per instance (depth, err): %s" % [(int(d), int(e)) for d, e in zip(depth, res.err)])
    return res


regs = pl.ids(S.GCP5[:5])
RATES = [0, 2, 10, 50, 100]
for r in RATES:
    report("configs[1] EPaxos n=5, %3d %%" % r, [S.spec(S.EPAXOS, 5, 2, regs, regs, commands_per_client=a.cmds,
                                                               conflict_rate=r, seed=20250213, instance=5 * i + k)
                                                        for k, r2 in enumerate(RATES) if r2 == r for i in range(a.seeds)])
regs3 = pl.ids(S.GCP5[:3])
report("configs[0] Atlas n=3 f=1", [S.spec(S.ATLAS, 3, 1, regs3, regs3, commands_per_client=a.cmds, conflict_rate=r,
                                           seed=20250213, instance=i) for i, r in enumerate(RATES * 8)])
for n, f in [(5, 1), (5, 2), (7, 1), (7, 2)]:
    subs = list(itertools.combinations(range(pl.R), n))[::a.stride]
    report("configs[2] Atlas n=%d f=%d" % (n, f), [S.spec(S.ATLAS, n, f, list(sub), list(sub), commands_per_client=100,
                                                         conflict_rate=2, seed=20250213, instance=i)
                                                  for i, sub in enumerate(subs)])


def far_planet(d, far_ms):
    """Processes pa, pb 40 ms apart, client regions ca, cb, cc (2 ms from the
    process of the same letter, 40 ms otherwise), and one region fNNN per entry
    of far_ms, NNN ms from everything."""
    names = ["pa", "pb", "ca", "cb", "cc"] + ["f%03d" % ms for ms in far_ms]
    for x in names:
        with open(os.path.join(d, x + ".dat"), "w") as f:
            for y in names:
                if x == y:
                    ms = 0.1
                elif x[0] == "f" or y[0] == "f":
                    ms = float(max(int(z[1:]) for z in (x, y) if z[0] == "f"))
                else:
                    ms = 2.0 if (x[0] != y[0] and x[1] == y[1]) else 40.0
                f.write("%.3f/%.3f/%.3f/0.100:%s\n" % (ms, ms, ms, y))
    return S.Planet(d)


if a.far:
    far_ms = list(range(40, 310, 10))
    with tempfile.TemporaryDirectory() as d:
        fp = far_planet(d, far_ms)
        for rate, cmds in ((0, 20), (100, 20), (100, 8)):
            print("far sweep, Atlas n=3 f=1, %d commands per client, GC off, conflicts %d %%, far region at %s ms"
                  % (cmds, rate, far_ms))
            report("  far sweep", [S.spec(S.ATLAS, 3, 1, fp.ids(["pa", "pb", "f%03d" % ms]), fp.ids(["ca", "cb", "cc"]),
                                          commands_per_client=cmds, conflict_rate=rate, gc_interval_ms=0, seed=61, instance=i)
                                   for i, ms in enumerate(far_ms)], planet=fp, each=True)
