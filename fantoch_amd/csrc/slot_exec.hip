// slot_exec.hip — the batched SlotExecutor of FPaxos (fx_slot_execute,
// fx_slot_run) and its stream generator (fx_slot_synth_generate).  The
// semantics: fantoch_amd.h; what is shared with the host twin (slot_host.cpp):
// fx_slot.h.
//
// k_slot_lane: a lane per stream, 64 streams per wavefront and workgroup, the
// shape the tiled planes were made for: one 16-byte load per lane fetches 4 rows
// of that lane's stream, and the 64 lanes read one 1 KiB tile.  A lane keeps
// `next` and a 64-bit bitmap of the waiting slots next .. next + 63 in
// registers; the arrival row of waiting slot s sits in word (s & 63) * 64 +
// lane of a ring in LDS (16 KiB per wavefront): a lane only ever touches its
// own column, whose words the 64 lanes find in 64 consecutive words, so no two
// lanes of a 32-lane half share a bank, and nothing orders lanes against each
// other.  A row whose slot lies at or beyond next + 64 stops the stream with
// FX_ERR_CAPACITY.  After a row the lane drains ctz(~bitmap) slots; the lanes'
// run lengths differ, and a lane with nothing to drain runs no trip of its own.
//
// k_slot_scan: a wavefront per stream and workgroup, any reordering, by the
// closed form of the semantics.  With T[s] = the first arrival row of slot s
// (pass A: a min-atomic per row), a row is bad if its slot is 0 or above
// `steps`, or if T[its slot] is another row (a repeat); f = the first bad row
// (the stream's length if none), whose kind is the stream's status.  The
// executed prefix is the longest run of slots 1 .. E with T[s] < f, and slot k
// <= E is released at the running maximum of T[1 .. k] (pass B: 64 slots per
// trip, lane i holding slot k0 + i, an inclusive max-scan over the lanes plus
// the carry of the trip before).  Pass C gives the rows below f whose slot is
// above E their FX_RELEASE_NONE: a pass of its own, so that no address is
// stored by two lanes in one launch.
//   T lives in `state`.  Its words are written by one lane (the clear, the
//   min-atomic) and read back by another of the same wavefront (the bad-row
//   check, pass B), so every access to T is an agent-scope relaxed atomic,
//   served at the L2 in the order the wavefront issued it: no plain load that
//   could hit a stale L1 line, no fence per element; one wavefront-scope fence
//   between the passes keeps the compiler from moving an access across them.
//   A stream's table belongs to its wavefront alone: nothing is handed from
//   one workgroup to another, there is no barrier and no spin loop.
//
// k_slot_synth: one thread per plane word (stream, i): slot i + 1 of the
// stream goes to the arrival row fx::slot_synth_row counts for it; a word that
// holds no slot is 0.  The rows of a stream's slots are a permutation of 0 ..
// L - 1, so every word of the plane is stored exactly once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "fantoch_amd.h"
#include "fx_internal.h"
#include "fx_slot.h"
#include "fx_wave.h"

namespace {

struct SArgs {
  fx_slot_batch in;
  fx_order_batch out;
  const uint32_t* stream_map;
  uint32_t num_lanes;
  uint32_t* state;
  uint32_t at_commit;
};

using fx::ctz64;
using fx::rl;

__global__ __launch_bounds__(64) void k_slot_lane(const SArgs a) {
  __shared__ uint32_t ring[64 * FX_SLOT_LANE_WINDOW];
  const uint32_t lane = threadIdx.x, l = blockIdx.x * 64u + lane, steps = a.in.steps;
  bool live = l < a.num_lanes;
  const uint32_t s = live ? (a.stream_map ? a.stream_map[l] : l) : 0u;
  live = live && s < a.in.num_streams;
  const uint32_t len = live ? fx::slot_length(a.in.lengths, s, steps) : 0u;
  // word of (row r, stream s): base + (r >> 2) * 256 + (r & 3)
  const size_t base = fx_index(0u, s, steps);
  const auto at = [base](uint32_t r) { return base + (size_t)(r >> 2) * 256u + (r & 3u); };
  uint32_t next = 1u, nexec = 0u, status = FX_OK;
  uint64_t waiting = 0ull;  // bit i: slot next + i waits

  const auto row = [&](uint32_t r, uint32_t slot) {
    if (r >= len || status) return;
    if (a.at_commit) {
      if (slot == 0u) {
        status = FX_ERR_SLOT;
        return;
      }
      a.out.order[at(nexec++)] = r | FX_ORDER_SCC_START;
      a.out.release[at(r)] = r;
      return;
    }
    status = fx::slot_row_status(slot, next, steps, FX_SLOT_LANE_WINDOW);
    if (status) return;
    const uint32_t d = slot - next;
    if ((waiting >> d) & 1ull) {
      status = FX_ERR_SLOT;
      return;
    }
    waiting |= 1ull << d;
    ring[(slot & 63u) * 64u + lane] = r;
    if (d != 0u) a.out.release[at(r)] = FX_RELEASE_NONE;
    const uint32_t n = ~waiting ? ctz64(~waiting) : 64u;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t w = ring[((next + i) & 63u) * 64u + lane];
      a.out.order[at(nexec + i)] = w | FX_ORDER_SCC_START;
      a.out.release[at(w)] = r;
    }
    next += n;
    nexec += n;
    waiting = n >= 64u ? 0ull : waiting >> n;
  };

  for (uint32_t r0 = 0; r0 < steps; r0 += 4u) {
    const bool act = r0 < len && !status;
    if (!__ballot(act)) break;
    if (act) {
      const uint4 q = *reinterpret_cast<const uint4*>(a.in.slot + at(r0));
      row(r0, q.x);
      row(r0 + 1u, q.y);
      row(r0 + 2u, q.z);
      row(r0 + 3u, q.w);
    }
  }
  if (live) {
    a.out.nexec[s] = nexec;
    a.out.err[s] = status;
  }
}

__device__ __forceinline__ uint32_t t_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(64) void k_slot_scan(const SArgs a) {
  const uint32_t blk = fx::xcd_slot(blockIdx.x), lane = threadIdx.x, steps = a.in.steps;
  if (blk >= a.num_lanes) return;
  const uint32_t s = a.stream_map ? a.stream_map[blk] : blk;
  if (s >= a.in.num_streams) return;
  const uint32_t len = fx::slot_length(a.in.lengths, s, steps);
  const uint32_t* const slot = a.in.slot;
  uint32_t status = FX_OK, E = 0u;

  if (a.at_commit) {
    for (uint32_t r0 = 0; r0 < len && !status; r0 += 64u) {
      const uint32_t r = r0 + lane;
      const uint64_t bad = __ballot(r < len && slot[fx_index(r, s, steps)] == 0u);
      const uint32_t f = bad ? r0 + ctz64(bad) : len;
      if (r < f) {
        a.out.order[fx_index(r, s, steps)] = r | FX_ORDER_SCC_START;
        a.out.release[fx_index(r, s, steps)] = r;
      }
      E = f < r0 + 64u ? f : r0 + 64u;
      if (bad) status = FX_ERR_SLOT;
    }
  } else {
    uint32_t* const T = a.state + (size_t)blk * ((steps + 63u) & ~63u);  // T[slot - 1]
    for (uint32_t i = lane; i < steps; i += 64u)
      __hip_atomic_store(&T[i], FX_RELEASE_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // pass A: the first arrival row of every slot
    for (uint32_t r = lane; r < len; r += 64u) {
      const uint32_t v = slot[fx_index(r, s, steps)];
      if (v - 1u < steps) __hip_atomic_fetch_min(&T[v - 1u], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // the first bad row and its kind
    uint32_t f = len;
    for (uint32_t r = lane; r < len && f == len; r += 64u) {
      const uint32_t v = slot[fx_index(r, s, steps)];
      if (v - 1u >= steps || t_load(&T[v - 1u]) != r) f = r;
    }
    f = fx::wave_min(f);
    if (f < len) {
      const uint32_t v = slot[fx_index(f, s, steps)];
      status = v > steps ? FX_ERR_CAPACITY : FX_ERR_SLOT;
    }
    // pass B: the executed prefix, 64 slots per trip
    uint32_t carry = 0u;
    for (uint32_t k0 = 0; k0 < f; k0 += 64u) {
      const uint32_t k = k0 + lane;
      const uint32_t t = k < steps ? t_load(&T[k]) : FX_RELEASE_NONE;
      const uint64_t absent = __ballot(t >= f);
      const uint32_t cnt = absent ? ctz64(absent) : 64u;
      uint32_t m = lane < cnt ? t : 0u;
#pragma unroll
      for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)m, o, 64);
        if (lane >= o) m = max(m, up);
      }
      m = max(m, carry);
      if (lane < cnt) {
        a.out.order[fx_index(k, s, steps)] = t | FX_ORDER_SCC_START;
        a.out.release[fx_index(t, s, steps)] = m;
      }
      E += cnt;
      if (cnt < 64u) break;
      carry = rl(m, 63u);
    }
    // pass C: the rows below f whose slot still waits
    for (uint32_t r = lane; r < f; r += 64u)
      if (slot[fx_index(r, s, steps)] > E) a.out.release[fx_index(r, s, steps)] = FX_RELEASE_NONE;
  }
  if (lane == 0) {
    a.out.nexec[s] = E;
    a.out.err[s] = status;
  }
}

__global__ __launch_bounds__(256) void k_slot_synth(uint64_t seed, uint32_t stream_base, const uint32_t* lengths,
                                                    uint32_t S, uint32_t steps, uint32_t window, uint32_t* out,
                                                    size_t plane) {
  const size_t w = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (w >= plane) return;
  uint32_t s = 0, slot = 0, row = 0;
  if (fx::slot_synth_word(w, seed, stream_base, lengths, S, steps, window, &s, &slot, &row))
    out[fx_index(row, s, steps)] = slot;
  else
    out[w] = 0u;
}

}  // namespace

using namespace fx;

extern "C" int fx_slot_execute(const fx_slot_batch* in, const fx_order_batch* out, const uint32_t* stream_map,
                               uint32_t num_lanes, uint32_t tier, void* state, uint32_t flags, void* hip_stream) {
  const int st = slot_check(in, out, flags);
  if (st) return st;
  if (tier > FX_SLOT_TIER_SCAN || (tier == FX_SLOT_TIER_SCAN) != (state != nullptr)) return FX_ERR_INVALID_ARG;
  if (!stream_map && num_lanes > in->num_streams) return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (num_lanes == 0) return FX_OK;
  if (num_lanes > 0x7FFFFFC0u) return FX_ERR_INVALID_ARG;
  const SArgs a{*in, *out, stream_map, num_lanes, (uint32_t*)state, (flags & FX_FLAG_EXECUTE_AT_COMMIT) ? 1u : 0u};
  hipStream_t hs = (hipStream_t)hip_stream;
  if (tier == FX_SLOT_TIER_SCAN)
    hipLaunchKernelGGL(k_slot_scan, dim3(xcd_grid(num_lanes)), dim3(64), 0, hs, a);
  else
    hipLaunchKernelGGL(k_slot_lane, dim3((num_lanes + 63u) / 64u), dim3(64), 0, hs, a);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}

// By default every stream at SCAN, which takes any reordering: at 20,480
// streams of 1,000 slots the LANE tier fills 320 wavefronts and is three times
// slower even where no stream leaves its window.  With
// FX_FLAG_FIRST_TIER(FX_SLOT_TIER_LANE) every stream at LANE, then the ones
// whose reordering left its window whole at SCAN.  The streams' statuses are in
// out->err; the return value is the call's own.
extern "C" int fx_slot_run(const fx_slot_batch* in, const fx_order_batch* out, uint32_t flags, void* hip_stream,
                           uint32_t* reruns) {
  if (reruns) *reruns = 0;
  const uint32_t first = (flags >> FX_FLAG_TIER_SHIFT) & 15u;  // 0: the default, else the tier + 1
  flags &= ~(15u << FX_FLAG_TIER_SHIFT);
  if (first > FX_SLOT_TIER_SCAN + 1u) return FX_ERR_INVALID_ARG;
  const int st0 = fx_slot_execute(in, out, nullptr, 0, FX_SLOT_TIER_LANE, nullptr, flags, hip_stream);
  if (st0) return st0;
  const std::vector<uint32_t> chain = first == FX_SLOT_TIER_LANE + 1u
                                          ? std::vector<uint32_t>{FX_SLOT_TIER_LANE, FX_SLOT_TIER_SCAN}
                                          : std::vector<uint32_t>{FX_SLOT_TIER_SCAN};
  const LadderRun r = run_ladder(
      in->num_streams, nullptr, out->err, (hipStream_t)hip_stream, chain, false,
      [&](uint32_t tier, uint32_t L) { return tier == FX_SLOT_TIER_SCAN ? fx_slot_state_bytes(in->steps, L) : (size_t)0; },
      [&](uint32_t tier, const uint32_t* map, uint32_t L, void* state) {
        return fx_slot_execute(in, out, map, L, tier, state, flags, hip_stream);
      });
  if (reruns) *reruns = r.reruns();
  return r.status;
}

extern "C" int fx_slot_synth_generate(uint64_t seed, uint32_t stream_base, uint32_t num_streams, uint32_t steps,
                                      const uint32_t* lengths, uint32_t window, uint32_t* slot_plane,
                                      void* hip_stream) {
  const int st = slot_synth_check(stream_base, num_streams, steps, window, slot_plane);
  if (st) return st;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  const size_t plane = fx_plane_words(num_streams, steps);
  if (plane == 0) return FX_OK;
  if (plane / 256u > 0x7FFFFFFFu) return FX_ERR_INVALID_ARG;
  hipLaunchKernelGGL(k_slot_synth, dim3((uint32_t)(plane / 256u)), dim3(256), 0, (hipStream_t)hip_stream, seed,
                     stream_base, lengths, num_streams, steps, window, slot_plane, plane);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}
