// pred_synth.hip — the Caesar commit-stream generator (fx_pred_synth.h) on the
// device, in two forms that write the same bytes:
//   k_pred_synth_tile     a workgroup takes a tile of 256 consecutive commands
//                         of one instance.  It draws the shared-key bit of the
//                         tile and its halo (n * horizon commands back,
//                         n * max_bump forward, to round borders) once, as
//                         ballot masks in LDS, and the n delivery jitters of
//                         the tile and of `window` commands either side once,
//                         a byte each.  Then a lane per command builds its dep
//                         row from the bits, counts its n ranks from the
//                         jitters and stores the row into its n streams.
//                         Consecutive workgroups take the same tile of
//                         consecutive instances, so the workgroups in flight
//                         together fill the same 64-stream plane tiles.
//   k_pred_synth_command  one thread per command, every bit and jitter drawn
//                         where it is looked at: the host twin's loop
//                         (pred_synth_emit), the form of k_synth.
// Both write about 1 TB/s on the bench shape (3.2 GB of 4-byte stores into the
// tiled planes): the stores bound the kernel, not the draws, and the tile form
// measured no faster (profiles/pred_synth.md has both times and the resource
// figures).  fx_pred_synth_generate runs the per-command form; the tile form
// stays selectable through fx_pred_synth_generate_form for measurement.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fantoch_amd.h"
#include "fx_internal.h"
#include "fx_pred_synth.h"

namespace fx {

constexpr uint32_t PS_TILE = 256;    // commands per workgroup = threads
constexpr uint32_t PS_WMAX = 64;     // windows up to this keep their jitters in LDS
constexpr uint32_t PS_BITS = 768;    // shared bits: tile + halo <= 256 + FX_PRED_MAX_DEPS + 7, in ballots of 64

template <bool LDSJ>
__global__ __launch_bounds__(256) void k_pred_synth_tile(fx_pred_synth_params p, uint32_t S, uint32_t steps,
                                                         uint32_t dmax, fx_pred_synth_planes pl, uint64_t items) {
  __shared__ uint32_t sh[PS_BITS / 32];
  __shared__ __attribute__((aligned(8))) uint8_t jit[LDSJ ? (PS_TILE + 2 * PS_WMAX) * 8 : 8];
  const uint32_t n = p.n, w = p.window, N = steps, tid = threadIdx.x;
  const size_t plane = fx_plane_words(S, steps);
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t local = (uint32_t)(item % p.instances);
    const uint32_t g0 = (uint32_t)(item / p.instances) * PS_TILE;
    const uint32_t g1 = g0 + PS_TILE < N ? g0 + PS_TILE : N;
    const PredSynthInstance ps = pred_synth_instance(p, local);
    // shared bits of the rounds [first round - horizon, last round + max_bump]
    const uint32_t r0 = g0 / n, r1 = (g1 - 1) / n + 1 + p.max_bump;
    const uint32_t b0 = (r0 > p.horizon ? r0 - p.horizon : 0u) * n;
    const uint32_t b1 = (r1 < ps.si.cmds ? r1 : ps.si.cmds) * n;
    for (uint32_t base = 0; base < b1 - b0; base += PS_TILE) {
      const uint32_t i = base + tid;
      const bool bit = i < b1 - b0 && synth_conflicts(ps.si, b0 + i);
      const uint64_t m = __ballot(bit);
      if ((tid & 63u) == 0) {
        sh[(i >> 5)] = (uint32_t)m;
        sh[(i >> 5) + 1] = (uint32_t)(m >> 32);
      }
    }
    // jitters of [g0 - w, g1 + w): byte q of word g = arrival key at process q + 1, less g
    const uint32_t a0 = g0 > w ? g0 - w : 0u;
    if constexpr (LDSJ) {
      const uint32_t a1 = g1 + w < N ? g1 + w : N;
      for (uint32_t i = tid; i < (a1 - a0) * n; i += PS_TILE) {
        const uint32_t g = a0 + i / n, q = i % n;
        jit[(g - a0) * 8 + q] = (uint8_t)(synth_arrival(ps.si, q + 1, g) - g);
      }
    }
    __syncthreads();
    const uint32_t g = g0 + tid;
    if (g < g1) {
      PredSynthRows rows;
      uint32_t arrival[8];
      if constexpr (LDSJ) {
        // synth_rank over the jitters in LDS
        const uint64_t* jw = reinterpret_cast<const uint64_t*>(jit);
        const uint64_t mine = jw[g - a0];
        const uint32_t lo = g > w ? g - w : 0u, hi = g + w < N - 1 ? g + w : N - 1;
        uint32_t rank[8];
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) rank[q] = lo;
        for (uint32_t g2 = lo; g2 <= hi; ++g2) {
          if (g2 == g) continue;
          const uint64_t other = jw[g2 - a0];
#pragma unroll
          for (uint32_t q = 0; q < 8; ++q) {
            const uint32_t a = g + (uint32_t)((mine >> (8 * q)) & 255u), a2 = g2 + (uint32_t)((other >> (8 * q)) & 255u);
            rank[q] += (a2 < a || (a2 == a && g2 < g)) ? 1u : 0u;
          }
        }
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
          arrival[q] = g + (uint32_t)((mine >> (8 * q)) & 255u);
          rows.at[q] = q < n ? fx_index(rank[q], local * n + q, steps) : 0;
        }
      } else {
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
          arrival[q] = 0;
          rows.at[q] = 0;
          if (q < n) {
            arrival[q] = synth_arrival(ps.si, q + 1, g);
            rows.at[q] = fx_index(synth_rank(ps.si, q + 1, g), local * n + q, steps);
          }
        }
      }
      const uint32_t mybit = (sh[(g - b0) >> 5] >> ((g - b0) & 31u)) & 1u;
      const uint32_t fg = mybit ? PRED_SYNTH_SHARED | pred_synth_bump(ps, g) : 0u;
      pred_synth_store(ps, g, fg, rows, arrival, plane, dmax, pl,
                       [&](uint32_t g2) { return (sh[(g2 - b0) >> 5] >> ((g2 - b0) & 31u)) & 1u; });
    }
    __syncthreads();  // the next tile's draws overwrite the LDS
  }
}

__global__ __launch_bounds__(256) void k_pred_synth_command(fx_pred_synth_params p, uint32_t S, uint32_t steps,
                                                            uint32_t dmax, fx_pred_synth_planes pl) {
  const size_t total = (size_t)p.instances * steps;
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x)
    pred_synth_emit(p, (uint32_t)(x / steps), (uint32_t)(x % steps), S, steps, dmax, pl);
}

}  // namespace fx

using namespace fx;

extern "C" {

int fx_pred_synth_generate_form(const fx_pred_synth_params* p, const fx_pred_synth_planes* planes, uint32_t form,
                                void* hip_stream) {
  uint32_t S, steps, dmax;
  int st = pred_synth_check(p, &S, &steps, &dmax);
  if (st) return st;
  st = pred_synth_check_planes(planes, dmax);
  if (st) return st;
  if (form > FX_PRED_SYNTH_FORM_COMMAND) return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  hipStream_t hs = (hipStream_t)hip_stream;
  if (form == FX_PRED_SYNTH_FORM_COMMAND) {
    const size_t total = (size_t)p->instances * steps;
    const uint32_t grid = (uint32_t)std::min<size_t>((total + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(k_pred_synth_command, dim3(grid), dim3(256), 0, hs, *p, S, steps, dmax, *planes);
  } else {
    const uint64_t items = (uint64_t)((steps + PS_TILE - 1) / PS_TILE) * p->instances;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(items, 1u << 20);
    if (p->window <= PS_WMAX)
      hipLaunchKernelGGL(k_pred_synth_tile<true>, dim3(grid), dim3(PS_TILE), 0, hs, *p, S, steps, dmax, *planes, items);
    else
      hipLaunchKernelGGL(k_pred_synth_tile<false>, dim3(grid), dim3(PS_TILE), 0, hs, *p, S, steps, dmax, *planes,
                         items);
  }
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}

int fx_pred_synth_generate(const fx_pred_synth_params* p, const fx_pred_synth_planes* planes, void* hip_stream) {
  return fx_pred_synth_generate_form(p, planes, FX_PRED_SYNTH_FORM_COMMAND, hip_stream);
}

}  // extern "C"
