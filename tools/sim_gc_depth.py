"""GC ring depth the Stable evaluation needs, from the FX_SIM_PROFILE build
(make prof): stat 47 of an instance is the deepest look-up of its gc_finish,
counted in ring entries from the newest back to the answer (rd + 1: the ring
had lost it).  Over the configs[1] mix (EPaxos n = 5, five conflict rates) and
over every --stride'th placement of configs[2] (Atlas n = 5 / 7, every region
subset), first launch only (tiered=False).

usage: FX_LIB=fantoch_amd/build_prof/libfantoch_amd.so python tools/sim_gc_depth.py [--seeds N] [--cmds M] [--stride K]"""
import argparse
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from fantoch_amd import sim as S

ap = argparse.ArgumentParser()
ap.add_argument("--seeds", type=int, default=256)
ap.add_argument("--cmds", type=int, default=1000)
ap.add_argument("--stride", type=int, default=7)
a = ap.parse_args()
assert os.environ.get("FX_LIB"), "set FX_LIB to the profile build"
pl = S.Planet()


def report(tag, specs):
    res = S.run(specs, pl, lat_cap=0, tiered=False)
    depth = res.stats[:, 47].astype(np.int64)
    hist = np.bincount(depth)
    print("%-28s %6d instances, errors %d, depth needed: max %d, histogram %s"
          % (tag, len(specs), int((res.err != 0).sum()), int(depth.max()), {i: int(c) for i, c in enumerate(hist) if c}))


regs = pl.ids(S.GCP5[:5])
report("configs[1] mix (EPaxos n=5)", [S.spec(S.EPAXOS, 5, 2, regs, regs, commands_per_client=a.cmds, conflict_rate=c,
                                             seed=20250213, instance=i)
                                      for i, c in enumerate([0, 2, 10, 50, 100] * a.seeds)])
for n, f in [(5, 1), (5, 2), (7, 1), (7, 2)]:
    subs = list(itertools.combinations(range(pl.R), n))[::a.stride]
    report("configs[2] Atlas n=%d f=%d" % (n, f), [S.spec(S.ATLAS, n, f, list(sub), list(sub), commands_per_client=a.cmds,
                                                         conflict_rate=2, seed=0, instance=i)
                                                  for i, sub in enumerate(subs)])
