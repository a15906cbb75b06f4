// fx_wave.h — the one-line wavefront helpers of the kernels (device only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fx {

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t rl(uint32_t v, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src);
}
__device__ __forceinline__ uint32_t gather(uint32_t v, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)v);
}
__device__ __forceinline__ uint64_t bal(bool p) { return (uint64_t)__ballot(p); }
__device__ __forceinline__ uint32_t ctz64(uint64_t m) { return (uint32_t)__builtin_ctzll(m); }
__device__ __forceinline__ uint32_t pop64(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }
__device__ __forceinline__ uint32_t pop32(uint32_t m) { return (uint32_t)__builtin_popcount(m); }

template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}
// the lowest v of the 64 lanes (all active): xor 1, xor 2 within a quad, the
// mirrors within 8 and within 16 lanes, then the four rows
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  v = min(v, dpp<0xB1>(v));   // quad_perm [1, 0, 3, 2]
  v = min(v, dpp<0x4E>(v));   // quad_perm [2, 3, 0, 1]
  v = min(v, dpp<0x141>(v));  // row_half_mirror
  v = min(v, dpp<0x140>(v));  // row_mirror
  return min(min(rl(v, 0), rl(v, 16)), min(rl(v, 32), rl(v, 48)));
}

}  // namespace fx
