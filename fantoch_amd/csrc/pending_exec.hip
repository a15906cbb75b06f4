// pending_exec.hip — AggregatePending for a batch (fx_pending_aggregate,
// fx_pending_run): a command's partials collected per rifl, one result row when
// the last has executed.  The semantics: fantoch_amd.h; what is shared with the
// host twin (pending_host.cpp): fx_pending.h.
//
// k_pending: one wavefront per stream and workgroup, 64 order rows per
// iteration, lane i holding row k0 + i.  What it does with a chunk, and the two
// places the live builders of a stream can sit, registers (ONCHIP) or buckets
// in the caller's state that the launch clears itself (HBM), are stated once,
// in pending_step.inc, for this kernel and the sessions' (pending_advance.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <vector>

#include "fantoch_amd.h"
#include "fx_internal.h"
#include "fx_pending.h"
#include "fx_wave.h"

namespace {

struct PArgs {
  fx_pending_batch in;
  fx_pending_out out;
  size_t plane;
  const uint32_t* stream_map;
  uint32_t num_lanes;
  uint4* state;
  uint32_t buckets;
};

#include "pending_step.inc"

template <bool HBM>
__global__ __launch_bounds__(64) void k_pending(const PArgs a) {
  const uint32_t blk = fx::xcd_slot(blockIdx.x), lane = threadIdx.x;
  if (blk >= a.num_lanes) return;
  const uint32_t s = a.stream_map ? a.stream_map[blk] : blk;
  if (s >= a.in.num_streams) return;
  const uint32_t steps = a.in.steps, ne = a.in.nexec[s], buckets = a.buckets;
  if (ne > steps) {
    if (lane == 0) {
      a.out.nready[s] = 0u;
      a.out.nopen[s] = 0u;
      a.out.err[s] = FX_ERR_ORDER_OVERFLOW;
    }
    return;
  }
  std::conditional_t<HBM, PendingBuckets<false>, PendingRegs> tab{};
  if constexpr (HBM) {
    tab = {a.state + (size_t)blk * buckets * 64u, buckets, steps};
    for (uint32_t i = lane; i < buckets * 64u; i += 64u) tab.tab[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  uint32_t nready = 0u, live = 0u, status = FX_OK;
  const uint64_t below = (1ull << lane) - 1ull;

  for (uint32_t k0 = 0; k0 < ne; k0 += 64u)
    if (!pending_chunk(a.in, a.out, a.plane, s, k0, ne, lane, below, tab, nready, live, status)) break;

  if (lane == 0) {
    a.out.nready[s] = nready;
    a.out.nopen[s] = live;
    a.out.err[s] = status;
  }
}

}  // namespace

using namespace fx;

extern "C" int fx_pending_aggregate(const fx_pending_batch* in, const fx_pending_out* out, const uint32_t* stream_map,
                                    uint32_t num_lanes, uint32_t tier, void* state, void* hip_stream) {
  const int st = pending_check(in, out, tier);
  if (st) return st;
  if ((tier == FX_PENDING_TIER_HBM) != (state != nullptr)) return FX_ERR_INVALID_ARG;
  if (!stream_map && num_lanes > in->num_streams) return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (num_lanes == 0) return FX_OK;
  if (num_lanes > 0x7FFFFFC0u) return FX_ERR_INVALID_ARG;
  const PArgs a{*in,       *out,          fx_plane_words(in->num_streams, in->steps), stream_map,
                num_lanes, (uint4*)state, pending_buckets(in->steps)};
  hipStream_t hs = (hipStream_t)hip_stream;
  const dim3 grid(xcd_grid(num_lanes));
  if (tier == FX_PENDING_TIER_HBM)
    hipLaunchKernelGGL(k_pending<true>, grid, dim3(64), 0, hs, a);
  else
    hipLaunchKernelGGL(k_pending<false>, grid, dim3(64), 0, hs, a);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}

// Every stream at ONCHIP, then the ones that ran out of builders whole at HBM.
// The streams' statuses are in out->err; the return value is the call's own.
extern "C" int fx_pending_run(const fx_pending_batch* in, const fx_pending_out* out, void* hip_stream,
                              uint32_t* reruns) {
  if (reruns) *reruns = 0;
  const int st0 = fx_pending_aggregate(in, out, nullptr, 0, FX_PENDING_TIER_ONCHIP, nullptr, hip_stream);
  if (st0) return st0;
  const LadderRun r = run_ladder(
      in->num_streams, nullptr, out->err, (hipStream_t)hip_stream, {FX_PENDING_TIER_ONCHIP, FX_PENDING_TIER_HBM}, false,
      [&](uint32_t tier, uint32_t L) {
        return tier == FX_PENDING_TIER_HBM ? fx_pending_state_bytes(in->steps, L) : (size_t)0;
      },
      [&](uint32_t tier, const uint32_t* map, uint32_t L, void* state) {
        return fx_pending_aggregate(in, out, map, L, tier, state, hip_stream);
      });
  if (reruns) *reruns = r.reruns();
  return r.status;
}
