// graph_metrics.hip — the metrics pass over a batch's order and release planes.
//
// Metrics::collect for ChainSize (one sample per SCC, mod.rs:492-493) and
// ExecutionDelay (t(release) - t(add), mod.rs:514-518).  One 256-thread block
// per (tile, 4-row block): thread t reads order word t of that 1 KiB granule.
// With one tile column of streams (S <= 64; configs[4]: 5) a block takes 256
// consecutive used words instead (4 S per 4-row block), not 4 S of 256 threads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fantoch_amd.h"
#include "fx_internal.h"
#include "fx_metrics.h"

namespace fx {

// Wave-aggregated histogram increment: one atomic per distinct bin in the wave
// (the leader lane adds the popcount of the lanes sharing its bin).  Most Adds
// of a wave land in one or two bins (ChainSize 1, small delays), so per-lane
// atomics serialised on one LDS address (PMC: 96 % of k_metrics' LDS cycles
// were bank-conflict cycles).  Called in wave-uniform control flow; bin ==
// kNoBin means "nothing to add" for that lane.
constexpr uint32_t kNoBin = 0xFFFFFFFFu;
__device__ inline void wave_hist_add(uint32_t* lds, unsigned long long* glob, uint32_t bin,
                                     uint32_t use_lds) {
  unsigned long long active = __ballot(bin != kNoBin);
  while (active) {
    const int leader = __ffsll((long long)active) - 1;
    const uint32_t b = (uint32_t)__shfl((int)bin, leader);
    const unsigned long long same = __ballot(bin == b);
    if ((int)__lane_id() == leader) {
      const uint32_t c = (uint32_t)__popcll(same);
      if (use_lds) atomicAdd(&lds[b], c);
      else atomicAdd(&glob[b], (unsigned long long)c);
    }
    active &= ~same;
  }
}

__global__ __launch_bounds__(256) void k_metrics(const uint32_t* __restrict__ hdr,
                                                 const uint32_t* __restrict__ order,
                                                 const uint32_t* __restrict__ release,
                                                 const uint32_t* __restrict__ nexec, uint32_t S,
                                                 uint32_t steps, unsigned long long* chain,
                                                 uint32_t nbc, unsigned long long* delay,
                                                 uint32_t nbd, uint32_t use_lds) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hist[];  // [nbc + nbd]
  const uint32_t steps4 = (steps + 3) >> 2;
  const uint32_t tiles = (S + 63) >> 6;
  const bool narrow = S <= 64;
  const uint32_t w = 4u * S;  // narrow: used words per 4-row block
  const size_t nblocks = narrow ? ((size_t)w * steps4 + 255) / 256 : (size_t)tiles * steps4;
  if (use_lds) {
    for (uint32_t q = threadIdx.x; q < nbc + nbd; q += blockDim.x) hist[q] = 0;
    __syncthreads();
  }
  const uint32_t t = threadIdx.x;
  // blk is block-uniform, so every wave runs the aggregated adds together
  // XCD-aware order (narrow batches): the hardware deals blocks to the 8 XCDs
  // round robin; each XCD taking a contiguous eighth of every grid pass keeps
  // the release / hdr lines its rows look up (nearby steps) in its own L2
  const size_t b0 = narrow && gridDim.x % 8u == 0 ? (size_t)(blockIdx.x % 8u) * (gridDim.x / 8u) + blockIdx.x / 8u
                                                  : blockIdx.x;
  for (size_t blk = b0; blk < nblocks; blk += gridDim.x) {
    uint32_t s, k;
    if (narrow) {
      const size_t it = blk * 256 + t;
      s = it < (size_t)w * steps4 ? (uint32_t)(it % w) >> 2 : S;
      k = (uint32_t)(it / w) * 4 + (t & 3);
    } else {
      s = (uint32_t)(blk / steps4) * 64 + (t >> 2);
      k = (uint32_t)(blk % steps4) * 4 + (t & 3);
    }
    uint32_t db = kNoBin, cb = kNoBin;
    // a count above `steps` is no count (fx_metrics.h): the stream gives no sample
    const uint32_t ne = s < S ? metrics_rows(nexec[s], steps) : 0;
    if (k < ne) {
      const uint32_t o = order[fx_index(k, s, steps)];
      const uint32_t rec = o & 0x7FFFFFFFu;
      const uint32_t rs = rec < steps ? release[fx_index(rec, s, steps)] : FX_RELEASE_NONE;
      if (rs < steps) {  // else not executed (errored stream)
        const uint32_t dl =
            FX_HDR_T(hdr[fx_index(rs, s, steps)]) - FX_HDR_T(hdr[fx_index(rec, s, steps)]);
        db = metrics_bin(dl, nbd);
        if (o & FX_ORDER_SCC_START) {
          uint32_t size = 1;
          while (k + size < ne && !(order[fx_index(k + size, s, steps)] & FX_ORDER_SCC_START)) ++size;
          cb = metrics_bin(size, nbc);
        }
      }
    }
    wave_hist_add(use_lds ? hist + nbc : nullptr, delay, db, use_lds);
    wave_hist_add(hist, chain, cb, use_lds);
  }
  if (use_lds) {
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < nbc + nbd; q += blockDim.x) {
      const uint32_t v = hist[q];
      if (v) {
        if (q < nbc) atomicAdd(&chain[q], (unsigned long long)v);
        else atomicAdd(&delay[q - nbc], (unsigned long long)v);
      }
    }
  }
}

}  // namespace fx

using namespace fx;

extern "C" int fx_batch_metrics(const fx_stream_batch* in, const fx_order_batch* out, const fx_hist_batch* h,
                                void* hip_stream) {
  const int st = metrics_check(in, out, h);
  if (st) return st;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  const uint32_t steps4 = (in->steps + 3) >> 2;
  const size_t nblocks = in->num_streams <= 64 ? ((size_t)4 * in->num_streams * steps4 + 255) / 256
                                               : (size_t)((in->num_streams + 63) / 64) * steps4;
  if (nblocks == 0) return FX_OK;
  const uint32_t grid = (uint32_t)std::min<size_t>(nblocks, 256 * 8);
  const size_t lds_bytes = (size_t)(h->nbins_chain + h->nbins_delay) * 4;
  const uint32_t use_lds = lds_bytes <= METRICS_LDS_BYTES ? 1u : 0u;
  hipLaunchKernelGGL(k_metrics, dim3(grid), dim3(256), use_lds ? lds_bytes : 0, (hipStream_t)hip_stream,
                     in->hdr, out->order, out->release, out->nexec, in->num_streams, in->steps,
                     (unsigned long long*)h->chain_size, h->nbins_chain,
                     (unsigned long long*)h->execution_delay, h->nbins_delay, use_lds);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}
