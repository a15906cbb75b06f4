// fx_pred_synth.h — seeded synthetic Caesar commit streams (host + device).
//
// Stands in for the commit streams Caesar hands its PredecessorsExecutor
// (PredecessorsExecutionInfo{dot, cmd, clock, deps}, fantoch_ps/src/protocol/
// caesar.rs MCommit -> executor/pred/executor.rs).  Instance, commands, keys
// and delivery are fx_synth.h's (synth_conflicts / synth_key / synth_arrival /
// synth_rank over its counter RNG); what differs is the clock and the deps.
// Per instance of n processes with one closed-loop client each:
//   * command g = (round j, coordinator s): dot (s, j), g = (j-1)*n + (s-1),
//     j = 1..cmds; key(g) = synth_key
//   * retry: B = max_bump, K = B + 1.  r(g) = 0 unless g is on the shared key,
//     B > 0 and draw % 100 < retry_pct for the draw (seed, instance, g,
//     PURPOSE_RETRY); then r(g) = 1 + (draw >> 32) % B, capped at cmds - j (a
//     cap to 0: not retried)
//   * clocks: proposal (K j, s); final = committed (K (j + r) + r, s).  The low
//     digit r keeps the final clocks of one source distinct, and a retry with
//     bump r passes every proposal through round j + r.  Packed (seq << 8) | s.
//   * deps (KeyClocks::predecessors at the quorum when g gets its final
//     timestamp: every conflicting command known with a lower timestamp):
//       { g2 != g : key(g2) == key(g), j2 >= max(1, j - horizon),
//                   proposal(g2) < final(g) lexicographically }
//     i.e. rounds [j - horizon, j) plus the lower sources of round j, and with
//     a bump r every same-key command through round j + r.  `horizon` stands
//     in for the GC of the key clocks.  Ascending by packed dot.
//     A dep whose own final clock is higher (it was retried further) is one
//     the executor waits for only to commit; one with a lower final clock
//     executes first.  Of two conflicting commands within the horizon the one
//     with the lower final clock is in the other's deps (Caesar's invariant),
//     and final clocks are a total order: a complete stream executes every
//     command.
//   * delivery: process p handles g at arrival key synth_arrival (t_ms), in
//     synth_rank order; the header's 5-bit deps field holds min(ndeps, 31).
// Not modelled: the wait condition (a proposal blocked behind a conflicting
// command with a higher timestamp that does not name it), recovery, and the
// per-process monotonicity of real clocks: a retried command of a source may
// end above that source's next proposal.
#pragma once
#include <stdint.h>

#include "fantoch_amd.h"
#include "fx_synth.h"

namespace fx {

enum : uint64_t { PURPOSE_RETRY = 5 };

constexpr uint32_t PRED_SYNTH_SHARED = 0x80000000u;  // flags word: on the shared key | bump r

struct PredSynthInstance {
  SynthInstance si;
  uint32_t max_bump, retry_pct;
};

FX_HD PredSynthInstance pred_synth_instance(const fx_pred_synth_params& p, uint32_t local) {
  PredSynthInstance ps;
  SynthInstance& si = ps.si;
  si.seed = p.seed;
  si.inst = p.instance_base + local;
  si.n = p.n;
  si.cmds = p.cmds_per_process;
  si.window = p.window;
  si.cycle_pct = 0;
  si.horizon = p.horizon;
  si.clients = 1;
  si.key_pool = 0;
  // the instance's conflict rate, chosen as synth_instance chooses it
  const uint32_t nc = p.num_conflicts ? p.num_conflicts : 1;
  const uint32_t ci = p.conflict_block ? (si.inst / p.conflict_block) % nc : si.inst % nc;
  si.conflict = p.conflict_pct[ci];
  ps.max_bump = p.max_bump;
  ps.retry_pct = p.retry_pct;
  return ps;
}

// The argument check of every entry point, and the shape.
inline int pred_synth_check(const fx_pred_synth_params* p, uint32_t* S, uint32_t* steps, uint32_t* dmax) {
  if (!p || p->n < 1 || p->n > 8 || p->cmds_per_process == 0 || p->instances == 0 || p->retry_pct > 100 ||
      p->num_conflicts > 8)
    return FX_ERR_INVALID_ARG;
  const uint64_t N = (uint64_t)p->n * p->cmds_per_process;
  if (N + p->window >= (1u << 24)) return FX_ERR_INVALID_ARG;
  const uint64_t d = (uint64_t)p->n * ((uint64_t)p->horizon + p->max_bump + 1u) - 1u;
  if (d > FX_PRED_MAX_DEPS) return FX_ERR_INVALID_ARG;
  if ((uint64_t)p->instance_base + p->instances >= (1ull << 32)) return FX_ERR_INVALID_ARG;
  if ((uint64_t)p->instances * p->n >= (1ull << 32)) return FX_ERR_INVALID_ARG;
  if (S) *S = p->instances * p->n;
  if (steps) *steps = (uint32_t)N;
  if (dmax) *dmax = (uint32_t)d;
  return FX_OK;
}
inline int pred_synth_check_planes(const fx_pred_synth_planes* pl, uint32_t dmax) {
  if (!pl || !pl->dot || !pl->hdr || !pl->deps || !pl->clock_lo || !pl->clock_hi) return FX_ERR_INVALID_ARG;
  if (!pl->ndeps && dmax > 31) return FX_ERR_INVALID_ARG;
  return FX_OK;
}

// Bump r(g) of a command g on the shared key (0: not retried).
FX_HD uint32_t pred_synth_bump(const PredSynthInstance& ps, uint32_t g) {
  if (ps.max_bump == 0 || ps.retry_pct == 0) return 0u;
  const uint64_t x = synth_rand(ps.si.seed, ps.si.inst, g, PURPOSE_RETRY);
  if ((uint32_t)(x % 100u) >= ps.retry_pct) return 0u;
  const uint32_t r = 1u + (uint32_t)((x >> 32) % ps.max_bump);
  const uint32_t left = ps.si.cmds - (g / ps.si.n + 1u);
  return r < left ? r : left;
}
// Flags of command g: PRED_SYNTH_SHARED | r(g) on the shared key, else 0.
FX_HD uint32_t pred_synth_flags(const PredSynthInstance& ps, uint32_t g) {
  return synth_conflicts(ps.si, g) ? PRED_SYNTH_SHARED | pred_synth_bump(ps, g) : 0u;
}

// Final (committed) clock of a command of round j by source s with bump r.
FX_HD uint64_t pred_synth_clock(const PredSynthInstance& ps, uint32_t j, uint32_t s, uint32_t r) {
  const uint64_t K = (uint64_t)ps.max_bump + 1u;
  return ((K * ((uint64_t)j + r) + r) << 8) | s;
}

// Deps of command g with flags fg, ascending by packed dot: emit(k, dot) for
// the k-th; on_shared(g2) answers synth_conflicts of another command of the
// instance (a candidate's proposal clock does not depend on its own retry).
// Returns their number.
template <class Shared, class Emit>
FX_HD uint32_t pred_synth_deps(const PredSynthInstance& ps, uint32_t g, uint32_t fg, Shared&& on_shared, Emit&& emit) {
  const uint32_t n = ps.si.n;
  const uint32_t s = g % n + 1, j = g / n + 1;
  const uint32_t shared = fg >> 31, r = fg & ~PRED_SYNTH_SHARED;
  const uint32_t lo = j > ps.si.horizon ? j - ps.si.horizon : 1u;
  uint32_t nd = 0;
  for (uint32_t s2 = 1; s2 <= n; ++s2) {
    if (!shared && s2 != s) continue;  // a private key: the own client's history alone
    // proposal (K j2, s2) < final (K (j + r) + r, s): with a bump every round
    // through j + r, else earlier rounds and the lower sources of round j
    const uint32_t hi = r ? j + r : (s2 < s ? j : j - 1);
    for (uint32_t j2 = lo; j2 <= hi; ++j2) {
      const uint32_t g2 = (j2 - 1) * n + (s2 - 1);
      if (g2 == g) continue;
      if ((uint32_t)on_shared(g2) == shared) emit(nd++, FX_PACK_DOT(s2, j2));
    }
  }
  return nd;
}

// Rows of command g in its n streams (stream = local * n + p - 1): at[p - 1].
struct PredSynthRows {
  size_t at[8];
};

// Writes command g of instance `local`, whose flags are fg and whose rows and
// arrival keys are known, into every plane: all dmax dep planes, unused slots 0.
template <class Shared>
FX_HD void pred_synth_store(const PredSynthInstance& ps, uint32_t g, uint32_t fg, const PredSynthRows& rows,
                            const uint32_t* arrival, size_t plane, uint32_t dmax, const fx_pred_synth_planes& pl,
                            Shared&& on_shared) {
  const uint32_t n = ps.si.n;
  uint32_t* deps = pl.deps;
  const uint32_t nd = pred_synth_deps(ps, g, fg, on_shared, [&](uint32_t k, uint32_t d) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t q = 0; q < 8; ++q)
      if (q < n) deps[(size_t)k * plane + rows.at[q]] = d;
  });
  for (uint32_t k = nd; k < dmax; ++k) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t q = 0; q < 8; ++q)
      if (q < n) deps[(size_t)k * plane + rows.at[q]] = 0u;
  }
  const uint32_t s = g % n + 1, j = g / n + 1;
  const uint64_t clock = pred_synth_clock(ps, j, s, fg & ~PRED_SYNTH_SHARED);
  const uint32_t d = FX_PACK_DOT(s, j);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t q = 0; q < 8; ++q)
    if (q < n) {
      const size_t at = rows.at[q];
      pl.dot[at] = d;
      pl.hdr[at] = FX_MAKE_HDR(arrival[q], nd < 31u ? nd : 31u, FX_KIND_ADD);
      pl.clock_lo[at] = (uint32_t)clock;
      pl.clock_hi[at] = (uint32_t)(clock >> 32);
      if (pl.ndeps) pl.ndeps[at] = nd;
    }
}

// One command, every flag and jitter drawn where it is looked at: the host
// twin's loop body, and the one-thread-per-command form of the kernel.
FX_HD void pred_synth_emit(const fx_pred_synth_params& p, uint32_t local, uint32_t g, uint32_t S, uint32_t steps,
                           uint32_t dmax, const fx_pred_synth_planes& pl) {
  const PredSynthInstance ps = pred_synth_instance(p, local);
  PredSynthRows rows;
  uint32_t arrival[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t q = 0; q < 8; ++q) {
    rows.at[q] = 0;
    arrival[q] = 0;
    if (q < ps.si.n) {
      rows.at[q] = fx_index(synth_rank(ps.si, q + 1, g), local * ps.si.n + q, steps);
      arrival[q] = synth_arrival(ps.si, q + 1, g);
    }
  }
  pred_synth_store(ps, g, pred_synth_flags(ps, g), rows, arrival, fx_plane_words(S, steps), dmax, pl,
                   [&](uint32_t g2) { return synth_conflicts(ps.si, g2); });
}

}  // namespace fx
