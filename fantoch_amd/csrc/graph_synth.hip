// graph_synth.hip — the synthetic commit-stream generator (fx_synth.h's
// synth_emit) on the device and its host twin.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "fantoch_amd.h"
#include "fx_internal.h"
#include "fx_synth.h"

namespace fx {

__global__ __launch_bounds__(256) void k_synth(fx_synth_params p, uint32_t S, uint32_t steps,
                                               uint32_t* dot, uint32_t* hdr, uint32_t* deps) {
  const uint32_t N = p.n * p.cmds_per_process;
  const size_t total = (size_t)p.instances * N;
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total;
       x += (size_t)gridDim.x * blockDim.x) {
    synth_emit(p, (uint32_t)(x / N), (uint32_t)(x % N), S, steps, dot, hdr, deps);
  }
}

}  // namespace fx

using namespace fx;

extern "C" {

static int check_synth(const fx_synth_params* p) {
  if (!p || p->n < 1 || p->n > 8 || p->cmds_per_process < 1 || p->instances < 1 ||
      p->num_conflicts > 8)
    return FX_ERR_INVALID_ARG;
  const uint64_t N = (uint64_t)p->n * p->cmds_per_process;
  if (p->cmds_per_process >= (1u << FX_SEQ_BITS) || N + p->window >= (1u << 24) ||
      N >= (1u << 26))
    return FX_ERR_INVALID_ARG;
  if ((uint64_t)p->instances * p->n >= (1ull << 32)) return FX_ERR_INVALID_ARG;
  if (p->clients > 1 && p->cmds_per_process % p->clients) return FX_ERR_INVALID_ARG;
  if (p->key_pool == 1 || (p->key_pool > 1 && p->clients > 1)) return FX_ERR_INVALID_ARG;
  return FX_OK;
}

int fx_synth_shape(const fx_synth_params* p, uint32_t* S, uint32_t* steps, uint32_t* dmax) {
  int st = check_synth(p);
  if (st) return st;
  if (S) *S = p->instances * p->n;
  if (steps) *steps = p->n * p->cmds_per_process;
  if (dmax) *dmax = p->n;
  return FX_OK;
}

int fx_synth_generate(const fx_synth_params* p, uint32_t* dot, uint32_t* hdr, uint32_t* deps,
                      void* hip_stream) {
  int st = check_synth(p);
  if (st) return st;
  if (!dot || !hdr || !deps) return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  const uint32_t S = p->instances * p->n, steps = p->n * p->cmds_per_process;
  hipStream_t hs = (hipStream_t)hip_stream;
  // zero the padding of the planes (tiles of 64 streams x 4 steps)
  const size_t plane = fx_plane_words(S, steps);
  if (hipMemsetAsync(dot, 0, plane * 4, hs) != hipSuccess) return FX_ERR_HIP;
  if (hipMemsetAsync(hdr, 0, plane * 4, hs) != hipSuccess) return FX_ERR_HIP;
  if (hipMemsetAsync(deps, 0, plane * 4 * p->n, hs) != hipSuccess) return FX_ERR_HIP;
  const size_t total = (size_t)p->instances * steps;
  const uint32_t grid = (uint32_t)std::min<size_t>((total + 255) / 256, 256 * 64);
  hipLaunchKernelGGL(k_synth, dim3(grid), dim3(256), 0, hs, *p, S, steps, dot, hdr, deps);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}

int fx_synth_generate_host(const fx_synth_params* p, uint32_t* dot, uint32_t* hdr, uint32_t* deps) {
  int st = check_synth(p);
  if (st) return st;
  if (!dot || !hdr || !deps) return FX_ERR_INVALID_ARG;
  const uint32_t S = p->instances * p->n, steps = p->n * p->cmds_per_process;
  const size_t plane = fx_plane_words(S, steps);
  memset(dot, 0, plane * 4);
  memset(hdr, 0, plane * 4);
  memset(deps, 0, plane * 4 * p->n);
  // every command writes its own words of the planes: commands split over threads
  const size_t total = (size_t)p->instances * steps;
  const uint32_t nt = total < 4096 ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (uint32_t t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      for (size_t i = t; i < total; i += nt)
        synth_emit(*p, (uint32_t)(i / steps), (uint32_t)(i % steps), S, steps, dot, hdr, deps);
    });
  for (auto& x : th) x.join();
  return FX_OK;
}

}  // extern "C"
