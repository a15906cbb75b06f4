// pred_exec.hip — Caesar's PredecessorsExecutor on the GPU: one wavefront per
// commit stream, the graph as LDS (or HBM) tables, many streams per launch.
//
// PredecessorsGraph (fantoch_ps/src/executor/pred/mod.rs:28-384,
// index.rs:10-120) needs no SCCs: a committed command waits (phase one) until
// every dep is committed, then (phase two) until every dep with a lower Caesar
// clock (seq, process id; common/pred/clocks/mod.rs:15-30) is executed; an
// execution completes the phase two of its waiters, recursively.  Tables:
//   vertex table  dot, arrival, clock (2 words), missing-deps count, deps
//                 (copied at commit) and, per phase, one bit per dep slot
//                 saying whether it is registered in that phase's PendingIndex
//   dot index     per source, seq mod Q -> vertex
//   clocks        committed and executed AEClocks: frontier + ring bitmap
//   recursion     frames (phase, waiter list, position) over a list stack:
//                 try_phase_one_pending / try_phase_two_pending run depth
//                 first exactly as the reference's recursive calls
// PendingIndex::remove(dep) is a lane-parallel scan of the vertex table
// (each vertex holds a dep at most once); the waiters are visited ascending
// by dot (the reference iterates a HashSet; canonical as C2 for the graph
// executor).  Outputs use the batched executor's planes: order row k =
// arrival index of the k-th executed command (every command its own group),
// release[arrival] = the step that executed it.
// The table layout (Lay), the tiers' layouts and the wavefront's executor (Pr)
// are in fx_pred.h, which the sessions (pred_advance.hip) and their host twin
// (pred_host.cpp) share; this file holds k_pred and the whole-stream entries.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fantoch_amd.h"
#include "fx_internal.h"

#include "fx_pred.h"

namespace fx {
namespace pred {

// FN / FD != 0 (the configs[1] shape, n = 5, dmax = 5): the SMALL tier with
// its layout compiled in -- table offsets become immediates, which frees the
// scalar registers the layout's fields held (the generic build spills about
// 50 SGPRs to VGPR lanes) -- and sized for occupancy: smaller tables
// (small_fixed_layout) and WPB streams per workgroup.  A CU holds at most 16
// workgroups, so one stream per workgroup stopped at 16 streams per CU
// whatever the tables; 4 per workgroup on 5.6 KB tables run 28.  Streams that
// outgrow the smaller tables rerun on the LDS tier as before.
template <bool HBM, uint32_t FN = 0, uint32_t FD = 0, uint32_t WPB = 1>
__global__ __launch_bounds__(64 * WPB) void k_pred(PArgs a, Lay Lrt) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const uint32_t wv = WPB > 1 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0u;
  const uint32_t li = xcd_slot(blockIdx.x) * WPB + wv;
  if (li >= a.k.num_lanes) return;  // whole wavefront
  Lay L = Lrt;
  if constexpr (FN != 0) {
    L = small_fixed_layout(FN, FD);
    a.k.n = FN;
    a.k.dmax = FD;
  }
  Pr<(WPB > 1)> w;
  w.a = a;
  w.L = L;
  w.lid = threadIdx.x & 63u;
  w.s = a.k.stream_map ? a.k.stream_map[li] : li;
  w.m = HBM ? a.k.state + (size_t)li * L.words : smem + wv * L.words;
  for (uint32_t i = w.lid; i < L.words; i += 64) w.m[i] = 0;
  w.sync();
  for (uint32_t i = w.lid; i < L.P; i += 64) w.m[L.vfree + i] = L.P - 1u - i;
  w.sync();
  w.nfree = L.P;
  const uint32_t len = a.k.lengths ? min(a.k.lengths[w.s], a.k.steps) : a.k.steps;
  uint32_t row = len ? w.row_load(0) : 0u, next = len > 4 ? w.row_load(4) : 0u;
  for (uint32_t r = 0; r < len && !w.err; ++r) {
    if (r && !(r & 3u)) {
      row = next;
      if (r + 4 < len) next = w.row_load(r + 4);
    }
    w.step = r;
    w.add(r, row);
  }
  if (w.lid == 0) {
    a.k.nexec[w.s] = w.nexec;
    a.k.err[w.s] = w.err;
  }
}

}  // namespace pred

}  // namespace fx

using namespace fx;

extern "C" size_t fx_pred_state_bytes(uint32_t n, uint32_t dmax, uint32_t lanes) {
  return (size_t)pred_layout(FX_PRED_TIER_HBM, std::max(n, 1u), dmax).words * 4 * lanes;
}

extern "C" int fx_pred_execute(const fx_pred_batch* in, const fx_order_batch* out, const uint32_t* stream_map,
                               uint32_t num_lanes, uint32_t tier, void* state, uint32_t flags,
                               void* hip_stream) {
  if (!in || !out || !in->base.dot || !in->base.hdr || (in->base.dmax && !in->base.deps) || !in->clock_lo ||
      !in->clock_hi || !out->order || !out->release || !out->nexec || !out->err)
    return FX_ERR_INVALID_ARG;
  if (in->base.n < 1 || in->base.n > 8 || in->base.dmax > FX_PRED_MAX_DEPS || in->base.steps >= (1u << 26) ||
      (!in->ndeps && in->base.dmax > 31))
    return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (!stream_map && num_lanes > in->base.num_streams) return FX_ERR_INVALID_ARG;
  if (tier > FX_PRED_TIER_HBM || (tier == FX_PRED_TIER_HBM) != (state != nullptr)) return FX_ERR_INVALID_ARG;
  if (num_lanes == 0) return FX_OK;
  const bool hbm = tier == FX_PRED_TIER_HBM;
  pred::PArgs a{};
  a.k = kargs_of(in->base, *out);
  a.k.stream_map = stream_map;
  a.k.num_lanes = num_lanes;
  a.k.state = (uint32_t*)state;
  a.k.flags = flags;
  a.clo = in->clock_lo;
  a.chi = in->clock_hi;
  a.ndeps = in->ndeps;
  const pred::Lay L = pred_layout(tier, in->base.n, in->base.dmax);
  hipStream_t hs = (hipStream_t)hip_stream;
  if (!hbm && L.words == 0) return FX_ERR_UNSUPPORTED;
  const uint32_t grid = xcd_grid(num_lanes);
  fx::profile_slot_record(FX_PROFILE_SLOT_PRED + tier, false, hs);
  if (hbm) {
    hipLaunchKernelGGL(pred::k_pred<true>, dim3(grid), dim3(64), 0, hs, a, L);
  } else {
    static bool configured = false;
    if (!configured) {
      (void)hipFuncSetAttribute((const void*)pred::k_pred<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024);
      (void)hipFuncSetAttribute((const void*)pred::k_pred<false, 5, 5, FX_PRED_WPB>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      configured = true;
    }
    if (tier == FX_PRED_TIER_SMALL && in->base.n == 5 && std::max(in->base.dmax, 1u) == 5) {
      const pred::Lay L5 = pred::small_fixed_layout(5, 5);
      constexpr uint32_t W = FX_PRED_WPB;
      hipLaunchKernelGGL((pred::k_pred<false, 5, 5, W>), dim3(xcd_grid((num_lanes + W - 1u) / W)), dim3(64 * W),
                         (size_t)L5.words * 4 * W, hs, a, L5);
    } else
      hipLaunchKernelGGL(pred::k_pred<false>, dim3(grid), dim3(64), (size_t)L.words * 4, hs, a, L);
  }
  if (hipGetLastError() != hipSuccess) return FX_ERR_HIP;
  fx::profile_slot_record(FX_PROFILE_SLOT_PRED + tier, true, hs);
  return FX_OK;
}

// Every stream at SMALL, then the ones that ran out of capacity at LDS, then
// HBM (tiers whose tables do not fit are skipped).  Synchronous.
extern "C" int fx_pred_run(const fx_pred_batch* in, const fx_order_batch* out, uint32_t flags, void* hip_stream,
                           uint32_t* reruns) {
  if (reruns) *reruns = 0;
  if (!in) return FX_ERR_INVALID_ARG;
  const uint32_t n = std::max(in->base.n, 1u), dmax = in->base.dmax;
  std::vector<uint32_t> chain;
  for (uint32_t tier = FX_PRED_TIER_SMALL; tier <= FX_PRED_TIER_HBM; ++tier)
    if (pred_layout(tier, n, dmax).words != 0) chain.push_back(tier);
  // the arguments and the device, checked by an empty launch at the first tier
  const int st0 = fx_pred_execute(in, out, nullptr, 0, chain[0], nullptr, flags, hip_stream);
  if (st0) return st0;
  const LadderRun r = run_ladder(
      in->base.num_streams, nullptr, out->err, (hipStream_t)hip_stream, chain, true,
      [&](uint32_t tier, uint32_t L) { return tier == FX_PRED_TIER_HBM ? fx_pred_state_bytes(n, dmax, L) : (size_t)0; },
      [&](uint32_t tier, const uint32_t* map, uint32_t L, void* state) {
        return fx_pred_execute(in, out, map, L, tier, state, flags, hip_stream);
      });
  if (r.status) return r.status;
  if (reruns) *reruns = r.reruns();
  return r.lowest;
}
