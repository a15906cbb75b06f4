// fx_ladder.hip — what the batched engines' drivers share: the device scratch
// that persists across calls and the capacity-rerun driver (run_ladder) behind
// fx_batch_run_tiered, fx_pred_run, fx_table_run* and fx_pending_run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fantoch_amd.h"
#include "fx_internal.h"

namespace fx {

static void* g_scratch[SCRATCH_SLOTS] = {};
static size_t g_scratch_cap[SCRATCH_SLOTS] = {};

void* scratch(uint32_t slot, size_t bytes) {
  if (slot >= SCRATCH_SLOTS) return nullptr;
  bytes = std::max<size_t>(bytes, 256);
  if (g_scratch_cap[slot] >= bytes) return g_scratch[slot];
  if (g_scratch[slot]) (void)hipFree(g_scratch[slot]);
  g_scratch[slot] = nullptr;
  g_scratch_cap[slot] = 0;
  const size_t grown = bytes + bytes / 4;
  if (hipMalloc(&g_scratch[slot], grown) != hipSuccess) return nullptr;
  g_scratch_cap[slot] = grown;
  return g_scratch[slot];
}

std::recursive_mutex& scratch_mutex() {
  static std::recursive_mutex m;
  return m;
}

// Streams of a launch (list, or 0..L-1 when list is null) that stopped with
// FX_ERR_CAPACITY, appended to out_list (order arbitrary: the next tier's
// stream map; results do not depend on it); cnt[0] = how many.
__global__ __launch_bounds__(256) void k_collect_capacity(const uint32_t* __restrict__ err,
                                                          const uint32_t* __restrict__ list, uint32_t L,
                                                          uint32_t* __restrict__ out_list, uint32_t* cnt) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t s = i < L ? (list ? list[i] : i) : 0u;
  const bool cap = i < L && err[s] == FX_ERR_CAPACITY;
  const uint64_t b = __ballot(cap);
  if (!b) return;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == (uint32_t)__builtin_ctzll(b)) base = atomicAdd(cnt, (uint32_t)__builtin_popcountll(b));
  base = (uint32_t)__shfl((int)base, (int)__builtin_ctzll(b), 64);
  if (cap) out_list[base + (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1ull))] = s;
}

// cnt[1] = lowest stream index (of list, or 0..L-1) with a nonzero status
__global__ __launch_bounds__(256) void k_first_error(const uint32_t* __restrict__ err,
                                                     const uint32_t* __restrict__ list, uint32_t L, uint32_t* cnt) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t s = i < L ? (list ? list[i] : i) : 0u;
  const bool bad = i < L && err[s] != 0;
  const uint64_t b = __ballot(bad);
  if (!b) return;
  uint32_t m = bad ? s : 0xFFFFFFFFu;
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) m = min(m, (uint32_t)__shfl_xor((int)m, (int)o, 64));
  if ((threadIdx.x & 63u) == 0) atomicMin(&cnt[1], m);
}

// Every decision stays on the device except one 4-byte read per tier: the
// streams that ran out of capacity are compacted into the next tier's stream
// map by k_collect_capacity, and the stream whose status a caller returns is
// found by k_first_error -- no per-stream host work, which at 4.4 M segments
// (configs[4]) had cost ~10 ms per call.
LadderRun run_ladder(uint32_t S, const std::vector<uint32_t>* only, const uint32_t* err, hipStream_t hs,
                     const std::vector<uint32_t>& chain, bool want_lowest, const LadderStateBytes& state_bytes,
                     const LadderLaunch& launch) {
  std::lock_guard<std::recursive_mutex> lock(scratch_mutex());
  LadderRun r;
  r.lanes.assign(chain.size(), 0u);
  const uint32_t L0 = only ? (uint32_t)only->size() : S;
  if (L0 == 0) return r;
  const auto failed = [&r](int st) {
    r.status = st;
    return r;
  };
  uint32_t* maps[2] = {(uint32_t*)scratch(SCRATCH_TIERED_MAP, (size_t)L0 * 4),
                       (uint32_t*)scratch(SCRATCH_TIERED_MAP2, (size_t)L0 * 4)};
  uint32_t* cnt = (uint32_t*)scratch(SCRATCH_TIERED_CNT, 8);
  if (!maps[0] || !maps[1] || !cnt) return failed(FX_ERR_HIP);
  if (only && hipMemcpyAsync(maps[0], only->data(), (size_t)L0 * 4, hipMemcpyHostToDevice, hs) != hipSuccess)
    return failed(FX_ERR_HIP);
  const uint32_t* list = only ? maps[0] : nullptr;  // the launch's streams: null = all S
  uint32_t L = L0, side = only ? 1u : 0u;
  uint32_t h[2] = {0, 0};
  for (size_t i = 0; i < chain.size() && L; ++i) {
    r.lanes[i] = L;
    const size_t bytes = state_bytes(chain[i], L);
    void* dstate = nullptr;
    if (bytes && !(dstate = scratch(SCRATCH_TIERED_STATE, bytes))) return failed(FX_ERR_HIP);
    const int st = launch(chain[i], list, L, dstate);
    if (st) return failed(st);
    uint32_t* next = maps[side];
    if (next == list) next = maps[side ^ 1u];
    if (hipMemsetAsync(cnt, 0, 4, hs) != hipSuccess) return failed(FX_ERR_HIP);
    hipLaunchKernelGGL(k_collect_capacity, dim3((L + 255) / 256), dim3(256), 0, hs, err, list, L, next, cnt);
    if (hipMemcpyAsync(h, cnt, 4, hipMemcpyDeviceToHost, hs) != hipSuccess || hipStreamSynchronize(hs) != hipSuccess)
      return failed(FX_ERR_HIP);
    L = h[0];
    list = next;
    side = (next == maps[0]) ? 1u : 0u;
  }
  if (!want_lowest) return r;
  // the lowest failing stream (streams still at FX_ERR_CAPACITY after the last
  // tier included)
  const uint32_t init[2] = {0, 0xFFFFFFFFu};
  if (hipMemcpyAsync(cnt, init, 8, hipMemcpyHostToDevice, hs) != hipSuccess) return failed(FX_ERR_HIP);
  if (only && hipMemcpyAsync(maps[0], only->data(), (size_t)L0 * 4, hipMemcpyHostToDevice, hs) != hipSuccess)
    return failed(FX_ERR_HIP);
  hipLaunchKernelGGL(k_first_error, dim3((L0 + 255) / 256), dim3(256), 0, hs, err, only ? maps[0] : nullptr, L0, cnt);
  uint32_t e = 0;
  if (hipMemcpyAsync(h, cnt, 8, hipMemcpyDeviceToHost, hs) != hipSuccess || hipStreamSynchronize(hs) != hipSuccess)
    return failed(FX_ERR_HIP);
  if (h[1] != 0xFFFFFFFFu && (hipMemcpyAsync(&e, err + h[1], 4, hipMemcpyDeviceToHost, hs) != hipSuccess ||
                              hipStreamSynchronize(hs) != hipSuccess))
    return failed(FX_ERR_HIP);
  r.lowest = (int)e;
  return r;
}

}  // namespace fx
