// pred_advance.hip — resumable streams of the predecessors executor
// (fx_pred_advance): k_pred's executor (Pr, fx_pred.h) continued from a saved
// state.  The semantics: fantoch_amd.h; the state layout, the argument check
// and the header check, shared with the host twin (pred_host.cpp): fx_pred.h.
//
// Between two Adds Pr's recursion is unwound (fsp == 0, ltop == 0), so what a
// stream carries from one call to the next is the tables below Lay::frames
// and six scalars: err, nexec, nfree, nreg0, nreg1 and the row reached.
//
// k_pred_advance: a wavefront per stream, WPB streams per workgroup (the
// mapping is k_pred's).  A call
//   1  reads the stream's header (every lane the same 12 words, one line) and,
//      without FX_FLAG_INIT, validates it (pred::header_ok) before anything of
//      it is used: a refused stream writes err[s] alone;
//   2  a stream with nothing to do (stopped earlier, or len <= done) writes
//      nexec[s] and err[s] (len < done: err[s] alone) and is done: its image
//      is never loaded;
//   3  SMALL / LDS: loads the image into LDS, 16 bytes per lane; HBM: uses it
//      in place.  With FX_FLAG_INIT the empty tables are built instead, as
//      k_pred builds them, and nothing of the old state is read;
//   4  runs rows [done, len) with k_pred's one-tile-ahead row_load, from the
//      tile that holds `done`;
//   5  stores the image back (not for a stream that stopped in this call: a
//      stopped stream's tables are not read again) and then the header.
// A stream's state belongs to its wavefront alone and is read before and
// written after everything else of the launch: plain vector loads and stores,
// no atomics, no barrier beyond Pr::sync(), no spin loop.  The copy loops are
// bounded by the image's words, the row loop by len <= steps, and every index
// into a table comes from a validated header or from Pr, whose bounds are
// k_pred's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fantoch_amd.h"
#include "fx_internal.h"
#include "fx_pred.h"

namespace fx {
namespace pred {

struct AArgs {
  PArgs p;
  uint32_t* state;
  uint32_t tier, init;
  uint32_t dmax_arg;  // the call's dmax as given (the compiled build overrides p.k.dmax)
};

template <bool HBM, uint32_t FN = 0, uint32_t FD = 0, uint32_t WPB = 1>
__global__ __launch_bounds__(64 * WPB) void k_pred_advance(AArgs aa, Lay Lrt) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const uint32_t wv = WPB > 1 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0u;
  const uint32_t s = xcd_slot(blockIdx.x) * WPB + wv;
  PArgs& a = aa.p;
  const uint32_t S = a.k.S;
  if (s >= S) return;  // whole wavefront
  Lay L = Lrt;
  if constexpr (FN != 0) {
    L = small_fixed_layout(FN, FD);
    a.k.n = FN;
    a.k.dmax = FD;
  }
  const uint32_t lid = threadIdx.x & 63u, steps = a.k.steps;
  const size_t iw = image_words(L, HBM ? FX_PRED_TIER_HBM : FX_PRED_TIER_SMALL);
  uint32_t* const H = aa.state + (size_t)s * H_WORDS;
  uint32_t* const img = aa.state + (size_t)S * H_WORDS + (size_t)s * iw;
  const uint32_t fixed = fixed_word(a.k.flags, a.ndeps != nullptr);
  const uint32_t len = session_length(a.k.lengths, s, steps);

  Pr<(WPB > 1)> w;
  w.a = a;
  w.L = L;
  w.lid = lid;
  w.s = s;
  w.m = HBM ? img : smem + wv * L.words;
  uint32_t done = 0;
  if (aa.init) {
    w.nfree = L.P;
  } else {
    uint32_t h[H_USED];
#pragma unroll
    for (uint32_t i = 0; i < H_USED; ++i) h[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)H[i]);
    if (!header_ok(h, steps, a.k.n, aa.dmax_arg, aa.tier, fixed, L.P)) {
      if (lid == 0) a.k.err[s] = FX_ERR_INVALID_ARG;
      return;
    }
    done = h[H_DONE];
    // a stream that stopped stays stopped; one with no new rows is done
    if (h[H_ERR] || len <= done) {
      if (lid == 0) {
        if (!h[H_ERR] && len < done) {
          a.k.err[s] = FX_ERR_INVALID_ARG;
        } else {
          a.k.nexec[s] = h[H_NEXEC];
          a.k.err[s] = h[H_ERR];
        }
      }
      return;
    }
    w.nexec = h[H_NEXEC];
    w.nfree = h[H_NFREE];
    w.nreg0 = h[H_NREG0];
    w.nreg1 = h[H_NREG1];
  }

  if (aa.init) {  // the empty tables, the free list as k_pred builds it
    const uint32_t nz = HBM ? L.frames : L.words;
    for (uint32_t i = lid; i < nz; i += 64) w.m[i] = 0;
    w.sync();
    for (uint32_t i = lid; i < L.P; i += 64) w.m[L.vfree + i] = L.P - 1u - i;
  } else if constexpr (!HBM) {
    if ((((uintptr_t)img) & 15u) == 0) {
      const uint4* const src = (const uint4*)img;
      uint4* const dst = (uint4*)w.m;
      for (uint32_t i = lid; i < L.frames / 4u; i += 64) dst[i] = src[i];
    } else {
      for (uint32_t i = lid; i < L.frames; i += 64) w.m[i] = img[i];
    }
  }
  w.sync();

  if (len > done) {
    const uint32_t r0 = done & ~3u;
    uint32_t row = w.row_load(r0), next = r0 + 4 < len ? w.row_load(r0 + 4) : 0u;
    for (uint32_t r = done; r < len && !w.err; ++r) {
      if (r != done && !(r & 3u)) {
        row = next;
        if (r + 4 < len) next = w.row_load(r + 4);
      }
      w.step = r;
      w.add(r, row);
    }
  }

  if constexpr (!HBM) {
    if (!w.err) {
      w.sync();
      if ((((uintptr_t)img) & 15u) == 0) {
        const uint4* const src = (const uint4*)w.m;
        uint4* const dst = (uint4*)img;
        for (uint32_t i = lid; i < L.frames / 4u; i += 64) dst[i] = src[i];
      } else {
        for (uint32_t i = lid; i < L.frames; i += 64) img[i] = w.m[i];
      }
    }
  }
  if (lid == 0) {
    H[H_TAG] = SESSION_TAG;
    H[H_STEPS] = steps;
    H[H_N] = a.k.n;
    H[H_DMAX] = aa.dmax_arg;
    H[H_TIER] = aa.tier;
    H[H_FIXED] = fixed;
    H[H_DONE] = len;
    H[H_ERR] = w.err;
    H[H_NEXEC] = w.nexec;
    H[H_NFREE] = w.nfree;
    H[H_NREG0] = w.nreg0;
    H[H_NREG1] = w.nreg1;
    a.k.nexec[s] = w.nexec;
    a.k.err[s] = w.err;
  }
}

}  // namespace pred
}  // namespace fx

using namespace fx;

extern "C" int fx_pred_advance(const fx_pred_batch* in, const fx_order_batch* out, uint32_t tier, void* state,
                               uint32_t flags, void* hip_stream) {
  const int st = pred_advance_check(in, out, tier, state, flags);
  if (st) return st;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  const uint32_t S = in->base.num_streams;
  if (S == 0u || in->base.steps == 0u) return FX_OK;
  if (S > 0x7FFFFFC0u) return FX_ERR_INVALID_ARG;
  const pred::Lay L = pred_session_layout(tier, in->base.n, in->base.dmax);
  if (L.words == 0) return FX_ERR_UNSUPPORTED;
  pred::AArgs a{};
  a.p.k = kargs_of(in->base, *out);
  a.p.k.flags = flags & FX_FLAG_EXECUTE_AT_COMMIT;
  a.p.clo = in->clock_lo;
  a.p.chi = in->clock_hi;
  a.p.ndeps = in->ndeps;
  a.state = (uint32_t*)state;
  a.tier = tier;
  a.init = (flags & FX_FLAG_INIT) ? 1u : 0u;
  a.dmax_arg = in->base.dmax;
  hipStream_t hs = (hipStream_t)hip_stream;
  static bool configured = false;
  if (!configured) {
    (void)hipFuncSetAttribute((const void*)pred::k_pred_advance<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipFuncSetAttribute((const void*)pred::k_pred_advance<false, 5, 5, FX_PRED_WPB>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    configured = true;
  }
  fx::profile_slot_record(FX_PROFILE_SLOT_PRED + 3u, false, hs);
  if (tier == FX_PRED_TIER_HBM) {
    hipLaunchKernelGGL(pred::k_pred_advance<true>, dim3(xcd_grid(S)), dim3(64), 0, hs, a, L);
  } else if (tier == FX_PRED_TIER_SMALL && in->base.n == 5 && std::max(in->base.dmax, 1u) == 5) {
    constexpr uint32_t W = FX_PRED_WPB;
    hipLaunchKernelGGL((pred::k_pred_advance<false, 5, 5, W>), dim3(xcd_grid((S + W - 1u) / W)), dim3(64 * W),
                       (size_t)L.words * 4 * W, hs, a, L);
  } else {
    hipLaunchKernelGGL(pred::k_pred_advance<false>, dim3(xcd_grid(S)), dim3(64), (size_t)L.words * 4, hs, a, L);
  }
  if (hipGetLastError() != hipSuccess) return FX_ERR_HIP;
  fx::profile_slot_record(FX_PROFILE_SLOT_PRED + 3u, true, hs);
  return FX_OK;
}
