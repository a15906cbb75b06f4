"""Cycles per simulator phase from the FX_SIM_PROFILE build (make prof).

usage: FX_LIB=fantoch_amd/build_prof/libfantoch_amd.so python tools/sim_phase.py [--seeds N] [--cmds M]
Prints, summed over instances, the shader-clock cycles (s_memtime ticks) spent
popping the next action, in each handler kind, in the executor, and in the
rest of the event, per event and per handler call; then the executor's search
counters (Adds that search, loop iterations by phase, searches decided at the
root, cycles in the loop), over all instances and per conflict rate."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from fantoch_amd import sim as S

ap = argparse.ArgumentParser()
ap.add_argument("--seeds", type=int, default=256)
ap.add_argument("--cmds", type=int, default=200)
ap.add_argument("--n", type=int, default=5)
ap.add_argument("--f", type=int, default=2)
ap.add_argument("--protocol", type=int, default=S.EPAXOS)
a = ap.parse_args()
assert os.environ.get("FX_LIB"), "set FX_LIB to the profile build"
pl = S.Planet()
regs = pl.ids(S.GCP5[:a.n])
specs = [S.spec(a.protocol, a.n, a.f, regs, regs, commands_per_client=a.cmds, conflict_rate=c,
                seed=20250213, instance=i) for i, c in enumerate([0, 2, 10, 50, 100] * a.seeds)]
res = S.run(specs, pl, lat_cap=0)
st = res.stats.astype(np.float64)
ev = st[:, 24].sum()
names = {0: "pop_min", 1: "run_event (all)", 2: "executor x_add", 3: "send_p", 4: "client R event", 5: "x_add load+check", 6: "note", 7: "run_handlers"}
kinds = ["MCollect", "MCollectAck", "MCommit", "MConsensus", "MConsensusAck", "x_add emit_one(fast)", "x_add x_store", "Submit"]
tot = st[:, 0].sum() + st[:, 1].sum()
print("events %d, cycles/event %.0f" % (ev, tot / ev))
for i in sorted(names):
    print("%-22s %8.0f cycles/event  %5.1f %%" % (names[i], st[:, i].sum() / ev, 100 * st[:, i].sum() / tot))
# run_event's pop of a process link (stat 39, inside "run_event (all)"); the
# deliveries are the handler calls of the five message kinds
dl = st[:, 16:21].sum()
print("%-22s %8.0f cycles/event  %5.1f %%  (%.0f cycles per delivery; deepest link %d)"
      % ("  pop of a P link", st[:, 39].sum() / ev, 100 * st[:, 39].sum() / tot, st[:, 39].sum() / max(dl, 1), st[:, 31].max()))
for k in range(8):
    c, n = st[:, 8 + k].sum(), st[:, 16 + k].sum()
    if n:
        print("  handler %-14s %8.0f cycles/call  %9d calls  %5.1f %%" % (kinds[k], c / n, n, 100 * c / tot))
# the handler loop itself (Sim::run_handlers_): iterations, the top-frame
# visit, and the popped frames by kind (stats 32..38 of a profile build)
it, vis, leaf, selfd = (st[:, 32 + i].sum() for i in range(4))
r0, r1, r2 = (st[:, 36 + i].sum() for i in range(3))
cmds = a.n * a.cmds * len(specs)  # one client per region
frames = leaf + selfd
if frames:
    loop = st[:, 7].sum() - st[:, 8:13].sum() - st[:, 15].sum() - st[:, 2].sum() - st[:, 3].sum()
    print("handler loop: %d iterations, %.2f per event, %.2f per command; frames %d (%.2f per command)"
          % (it, it / ev, it / cmds, frames, frames / cmds))
    print("  top-frame visit        %8.0f cycles/event  %5.1f %%  (%.0f cycles per frame)" % (vis / ev, 100 * vis / tot, vis / frames))
    print("  loop net of handlers, x_add and sends %8.0f cycles/event  %5.1f %%" % (loop / ev, 100 * loop / tot))
    print("  frames: leaf %.1f %%, handing a self-delivery on %.1f %%; ready results 0: %.1f %%, 1: %.1f %%, more: %.2f %% (%d frames)"
          % (100 * leaf / frames, 100 * selfd / frames, 100 * r0 / frames, 100 * r1 / frames, 100 * r2 / frames, r2))
rates = np.array([0, 2, 10, 50, 100] * a.seeds)


def search(m, tag):
    """The executor's search (stats 40..46 of a profile build: two 32-bit counts
    per word) over the instances selected by m."""
    raw = res.stats[m, 40:47].astype(np.uint64)
    lo = (raw & np.uint64(0xFFFFFFFF)).sum(axis=0).astype(np.float64)
    hi = (raw >> np.uint64(32)).sum(axis=0).astype(np.float64)
    adds, tries = lo[0], hi[0]
    dfs, skips, tryi, chk = lo[1], hi[1], lo[2], hi[2]
    add_miss, try_single, try_miss, past = lo[3], hi[3], lo[4], hi[4]
    stale, loops = lo[5], hi[5]
    cyc = st[m, 46].sum()
    tr = st[m, 0].sum() + st[m, 1].sum()
    searches = adds + tries
    if not searches:
        print("%s: no Add searches" % tag)
        return
    it = dfs + tryi + chk
    print("%s: Adds that search %d (%.1f %% of %d Adds), retried waiters searched %d, Adds in the loop %d"
          % (tag, adds, 100 * adds / max(st[m, 22].sum(), 1), st[m, 22].sum(), tries, loops))
    print("  loop iterations %d: dfs %d (skip-only %d, %.1f %%), try %d, check %d; %.2f per searching Add"
          % (it, dfs, skips, 100 * skips / max(dfs, 1), tryi, chk, it / max(adds, 1)))
    print("  root-decided: first Adds filed under a missing dep %d (%.1f %% of searching Adds); retried waiters with"
          " no unexecuted dep %d, with a missing first dep %d (%.1f %% of retries); together %.1f %% of %d searches"
          % (add_miss, 100 * add_miss / max(adds, 1), try_single, try_miss,
             100 * (try_single + try_miss) / max(tries, 1), 100 * (add_miss + try_single + try_miss) / searches,
             searches))
    print("  walks started past skipped deps %d, kept deps found executed when reached %d" % (past, stale))
    print("  cycles in the loop %.3g, %.1f %% of all, %.0f per Add in the loop" % (cyc, 100 * cyc / tr, cyc / max(loops, 1)))


search(np.ones(len(rates), dtype=bool), "search, all")
for r in [0, 2, 10, 50, 100]:
    search(rates == r, "search, conflict %3d%%" % r)
# per conflict rate: cycles per instance and the executor's share
for r in [0, 2, 10, 50, 100]:
    m = rates == r
    tr = st[m, 0].sum() + st[m, 1].sum()
    print("conflict %3d%%: %.3g cycles/instance, events/instance %.0f, executor %.1f %%, handlers %.1f %%, send_p %.1f %%"
          % (r, tr / m.sum(), st[m, 24].sum() / m.sum(), 100 * st[m, 2].sum() / tr,
             100 * st[m, 8:16].sum() / tr, 100 * st[m, 3].sum() / tr))
