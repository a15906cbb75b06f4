// pred_host.cpp — the host twin of the predecessors executor's sessions
// (fx_pred_advance_host) and fx_pred_session_bytes, which needs no device.
// A serial statement of PredecessorsGraph (fantoch_ps/src/executor/pred/
// mod.rs:104-383, index.rs:96-120) with the limits of the device tables: the
// limits come from the shared Lay / pred_layout (fx_pred.h) and are counted
// as k_pred counts them --
//   vertices  a commit with P commands pending
//   index     a commit whose seq mod Q is that of a pending dot of its source
//   window    a commit / an execution with seq - frontier - 1 >= 32 WB
//   frames    a PendingIndex::remove at recursion depth FD while that phase's
//             index holds any registration (tested before the removal)
//   lists     the waiter sets of all live frames together exceed LL entries
// -- and the waiters of a removal are visited ascending by dot.  Where the
// device runs a frame stack over LDS lists, this is the reference's recursion
// with a depth and a live-waiter count; where the device scans the vertex table
// lane-parallel and rank-sorts, this collects and std::sorts.  The state is the
// twin's own: the shared header, then per stream the tables below Lay::frames
// as plain arrays (the recursion keeps nothing between two Adds).
// No HIP call in here, so the file also builds alone with a host compiler
// (tests/cpp/pred_advance_host_check.cpp under the sanitizers).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <algorithm>
#include <thread>
#include <vector>

#include "fx_pred.h"

namespace {

using fx::pred::Lay;
constexpr uint32_t NONE = fx::pred::NONE;

struct Graph {
  const fx_pred_batch& in;
  const fx_order_batch& out;
  Lay L;
  uint32_t* m;  // the tables [0, L.frames)
  uint32_t s, steps, dmax, at_commit;
  uint32_t err = 0, nfree = 0, nexec = 0, nreg[2] = {0, 0}, step = 0;
  uint32_t depth = 0, live = 0;  // live frames and their waiters

  size_t ix(uint32_t r) const { return fx_index(r, s, steps); }
  uint32_t& reg(uint32_t ph, uint32_t v, uint32_t j) { return m[L.vreg + (ph * L.P + v) * L.DW + (j >> 5)]; }

  // AEClock: a frontier per source and a ring bitmap of the seqs above it
  bool contains(uint32_t front, uint32_t bits, uint32_t d) const {
    const uint32_t src = FX_DOT_SRC(d), sq = FX_DOT_SEQ(d);
    if (src < 1 || src > L.n) return false;
    const uint32_t f = m[front + src - 1];
    if (sq <= f) return true;
    if (sq - f - 1 >= L.WB * 32u) return false;
    const uint32_t b = sq & (L.WB * 32u - 1u);
    return (m[bits + (src - 1) * L.WB + (b >> 5)] >> (b & 31u)) & 1u;
  }
  void clock_add(uint32_t front, uint32_t bits, uint32_t d) {
    const uint32_t src = FX_DOT_SRC(d), sq = FX_DOT_SEQ(d);
    if (src < 1 || src > L.n) { err = FX_ERR_DOT_RANGE; return; }
    uint32_t f = m[front + src - 1];
    if (sq <= f) return;
    if (sq - f - 1 >= L.WB * 32u) { err = FX_ERR_CAPACITY; return; }
    const uint32_t mask = L.WB * 32u - 1u;
    uint32_t* const ring = m + bits + (src - 1) * L.WB;
    ring[(sq & mask) >> 5] |= 1u << (sq & 31u);
    while ((ring[((f + 1) & mask) >> 5] >> ((f + 1) & 31u)) & 1u) {
      ring[((f + 1) & mask) >> 5] &= ~(1u << ((f + 1) & 31u));
      ++f;
    }
    m[front + src - 1] = f;
  }

  uint32_t hslot(uint32_t d) const { return (FX_DOT_SRC(d) - 1) * L.Q + (FX_DOT_SEQ(d) & (L.Q - 1u)); }
  uint32_t find(uint32_t d) const {
    const uint32_t src = FX_DOT_SRC(d);
    if (src < 1 || src > L.n) return NONE;
    const uint32_t v = m[L.hidx + hslot(d)];
    return (v != 0 && m[L.vdot + v - 1] == d) ? v - 1 : NONE;
  }
  uint64_t clock_of(uint32_t v) const { return ((uint64_t)m[L.vchi + v] << 32) | m[L.vclo + v]; }

  // execute (mod.rs:369-383)
  void execute(uint32_t d, uint32_t rec) {
    clock_add(L.efront, L.ebits, d);
    if (err) return;
    if (nexec >= steps) { err = FX_ERR_ORDER_OVERFLOW; return; }
    out.order[ix(nexec)] = rec | FX_ORDER_SCC_START;
    out.release[ix(rec)] = step;
    ++nexec;
  }

  // try_phase_one_pending / try_phase_two_pending (mod.rs:295-339) over
  // PendingIndex::remove(d) (index.rs:117-119)
  void try_pending(uint32_t ph, uint32_t d) {
    if (nreg[ph] == 0) return;  // an empty index: no frame
    if (depth >= L.FD) { err = FX_ERR_CAPACITY; return; }
    std::vector<uint32_t> waiters;
    for (uint32_t v = 0; v < L.P; ++v) {
      if (m[L.vdot + v] == 0) continue;
      const uint32_t nd = m[L.vnd + v];
      for (uint32_t j = 0; j < nd; ++j)
        if (((reg(ph, v, j) >> (j & 31u)) & 1u) && m[L.vdeps + v * L.D + j] == d) {
          reg(ph, v, j) &= ~(1u << (j & 31u));
          waiters.push_back(m[L.vdot + v]);
          break;
        }
    }
    const uint32_t cnt = (uint32_t)waiters.size();
    nreg[ph] -= cnt;
    if (!cnt) return;
    if (live + cnt > L.LL) { err = FX_ERR_CAPACITY; return; }
    std::sort(waiters.begin(), waiters.end());
    ++depth;
    live += cnt;
    for (uint32_t i = 0; i < cnt && !err; ++i) {
      const uint32_t p = waiters[i], v = find(p);
      if (v == NONE || m[L.vmiss + v] == 0) { err = FX_ERR_CAPACITY; return; }
      if (--m[L.vmiss + v] == 0) {
        if (ph == 0) move_to_phase_two(p, v);
        else save_to_execute(p, v);
      }
    }
    --depth;
    live -= cnt;
  }

  // save_to_execute (mod.rs:341-367)
  void save_to_execute(uint32_t d, uint32_t v) {
    const uint32_t rec = m[L.vrec + v];
    m[L.hidx + hslot(d)] = 0;
    m[L.vdot + v] = 0;
    m[L.vfree + nfree++] = v;
    execute(d, rec);
    if (err) return;
    try_pending(1, d);
  }

  // move_to_phase_two (mod.rs:208-275)
  void move_to_phase_two(uint32_t d, uint32_t v) {
    const uint64_t cv = clock_of(v);
    const uint32_t nd = m[L.vnd + v];
    uint32_t miss = 0;
    for (uint32_t j = 0; j < nd; ++j) {
      const uint32_t dep = m[L.vdeps + v * L.D + j];
      if (contains(L.efront, L.ebits, dep)) continue;
      const uint32_t w = find(dep);
      if (w == NONE) { err = FX_ERR_CAPACITY; return; }  // "non-executed dependency must exist"
      if (clock_of(w) < cv) {
        reg(1, v, j) |= 1u << (j & 31u);
        ++miss;
      }
    }
    nreg[1] += miss;
    if (miss) m[L.vmiss + v] = miss;
    else save_to_execute(d, v);
  }

  // move_to_phase_one (mod.rs:154-206)
  void move_to_phase_one(uint32_t d, uint32_t v) {
    const uint32_t nd = m[L.vnd + v];
    uint32_t miss = 0;
    for (uint32_t j = 0; j < nd; ++j)
      if (!contains(L.cfront, L.cbits, m[L.vdeps + v * L.D + j])) {
        reg(0, v, j) |= 1u << (j & 31u);
        ++miss;
      }
    nreg[0] += miss;
    if (miss) m[L.vmiss + v] = miss;
    else move_to_phase_two(d, v);
  }

  // add (mod.rs:104-152)
  void add(uint32_t r) {
    const size_t at = ix(r);
    const uint32_t d = in.base.dot[at];
    const uint32_t src = FX_DOT_SRC(d);
    if (src < 1 || src > L.n || FX_DOT_SEQ(d) == 0) { err = FX_ERR_DOT_RANGE; return; }
    if (contains(L.cfront, L.cbits, d)) { err = FX_ERR_DOUBLE_INDEX; return; }  // mod.rs:123
    clock_add(L.cfront, L.cbits, d);
    if (err) return;
    if (at_commit) {
      execute(d, r);
      return;
    }
    const uint32_t h = hslot(d), old = m[L.hidx + h];
    if (old != 0) {
      err = m[L.vdot + old - 1] == d ? FX_ERR_DOUBLE_INDEX : FX_ERR_CAPACITY;
      return;
    }
    if (!nfree) { err = FX_ERR_CAPACITY; return; }
    const uint32_t v = m[L.vfree + --nfree];
    const uint32_t nd = std::min(in.ndeps ? in.ndeps[at] : FX_HDR_ND(in.base.hdr[at]), dmax);
    m[L.vdot + v] = d;
    m[L.vrec + v] = r;
    m[L.vclo + v] = in.clock_lo[at];
    m[L.vchi + v] = in.clock_hi[at];
    m[L.vmiss + v] = 0;
    m[L.vnd + v] = nd;
    for (uint32_t ph = 0; ph < 2; ++ph)
      for (uint32_t k = 0; k < L.DW; ++k) m[L.vreg + (ph * L.P + v) * L.DW + k] = 0;
    const size_t plane = fx_plane_words(in.base.num_streams, steps);
    for (uint32_t j = 0; j < nd; ++j) m[L.vdeps + v * L.D + j] = in.base.deps[(size_t)j * plane + at];
    m[L.hidx + h] = v + 1;
    try_pending(0, d);  // mod.rs:136
    if (err) return;
    move_to_phase_one(d, v);  // mod.rs:139
  }
};

void advance_stream(const fx_pred_batch& in, const fx_order_batch& out, uint32_t tier, uint32_t* state, bool init,
                    uint32_t at_commit, const Lay& L, uint32_t s) {
  using namespace fx::pred;
  const uint32_t S = in.base.num_streams, steps = in.base.steps;
  uint32_t* const H = state + (size_t)s * H_WORDS;
  uint32_t* const img = state + (size_t)S * H_WORDS + (size_t)s * image_words(L, tier);
  const uint32_t fixed = fixed_word(at_commit ? FX_FLAG_EXECUTE_AT_COMMIT : 0u, in.ndeps != nullptr);
  const uint32_t len = session_length(in.base.lengths, s, steps);
  Graph g{in, out, L, img, s, steps, in.base.dmax, at_commit};
  uint32_t done = 0;
  if (init) {
    std::fill(img, img + L.frames, 0u);
    for (uint32_t i = 0; i < L.P; ++i) img[L.vfree + i] = L.P - 1u - i;
    g.nfree = L.P;
  } else {
    if (!header_ok(H, steps, in.base.n, in.base.dmax, tier, fixed, L.P)) {
      out.err[s] = FX_ERR_INVALID_ARG;
      return;
    }
    done = H[H_DONE];
    if (H[H_ERR] || len <= done) {
      if (!H[H_ERR] && len < done) {
        out.err[s] = FX_ERR_INVALID_ARG;
      } else {
        out.nexec[s] = H[H_NEXEC];
        out.err[s] = H[H_ERR];
      }
      return;
    }
    g.nexec = H[H_NEXEC], g.nfree = H[H_NFREE], g.nreg[0] = H[H_NREG0], g.nreg[1] = H[H_NREG1];
  }
  for (uint32_t r = done; r < len && !g.err; ++r) {
    g.step = r;
    g.add(r);
  }
  H[H_TAG] = SESSION_TAG, H[H_STEPS] = steps, H[H_N] = in.base.n, H[H_DMAX] = in.base.dmax, H[H_TIER] = tier;
  H[H_FIXED] = fixed, H[H_DONE] = len, H[H_ERR] = g.err, H[H_NEXEC] = g.nexec, H[H_NFREE] = g.nfree;
  H[H_NREG0] = g.nreg[0], H[H_NREG1] = g.nreg[1];
  out.nexec[s] = g.nexec;
  out.err[s] = g.err;
}

}  // namespace

extern "C" {

size_t fx_pred_session_bytes(uint32_t tier, uint32_t n, uint32_t dmax, uint32_t num_streams) {
  if (tier > FX_PRED_TIER_HBM || n < 1 || n > 8 || dmax > FX_PRED_MAX_DEPS) return 0;
  const Lay L = fx::pred_session_layout(tier, n, dmax);
  if (L.words == 0) return 0;
  return (size_t)num_streams * ((size_t)fx::pred::H_WORDS + fx::pred::image_words(L, tier)) * 4u;
}

int fx_pred_advance_host(const fx_pred_batch* in, const fx_order_batch* out, uint32_t tier, void* state,
                         uint32_t flags) {
  const int st = fx::pred_advance_check(in, out, tier, state, flags);
  if (st) return st;
  const uint32_t S = in->base.num_streams;
  if (S == 0u || in->base.steps == 0u) return FX_OK;
  const Lay L = fx::pred_session_layout(tier, in->base.n, in->base.dmax);
  if (L.words == 0) return FX_ERR_UNSUPPORTED;
  const bool init = (flags & FX_FLAG_INIT) != 0u;
  const uint32_t at_commit = (flags & FX_FLAG_EXECUTE_AT_COMMIT) ? 1u : 0u;
  // streams are independent: up to 16 threads, each a contiguous share
  const uint32_t nt = S < 64 ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  auto share = [&](uint32_t t) {
    for (uint32_t s = (uint32_t)((uint64_t)S * t / nt); s < (uint32_t)((uint64_t)S * (t + 1) / nt); ++s)
      advance_stream(*in, *out, tier, (uint32_t*)state, init, at_commit, L, s);
  };
  if (nt == 1) {
    share(0);
  } else {
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < nt; ++t) th.emplace_back(share, t);
    for (auto& x : th) x.join();
  }
  return FX_OK;
}

}  // extern "C"
