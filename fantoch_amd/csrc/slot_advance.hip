// slot_advance.hip — resumable streams of the slot executor (fx_slot_advance):
// k_slot_scan's closed form (slot_exec.hip) continued from a saved state.  The
// semantics: fantoch_amd.h; the state layout, the argument check and the
// header check, shared with the host twin (slot_host.cpp): fx_slot.h.
//
// k_slot_advance: a wavefront per stream and workgroup.  Per stream the state
// is a header {tag | commit flag, steps, done, E, carry, err} and T[slot - 1] =
// the first arrival row of the slot, which the session keeps: FX_FLAG_INIT
// clears it, no later call does.  A call runs rows [done, len):
//   pass A  a min-atomic of the row into T[slot - 1] for 1 <= slot <= steps.
//           A slot that arrived in an earlier call holds a row below done,
//           which wins.
//   f       the wave-minimum bad row of [done, len), len if there is none: a
//           row whose slot is 0 or above `steps`, or whose T entry is another
//           row (a repeat, of a slot of this call or of one executed or
//           waiting since an earlier call).  Its kind is the stream's status.
//   pass B  from slot index E, the executed prefix the calls before left, not
//           from 0: 64 slots per trip, an entry at or above f counts as
//           absent, the inclusive max-scan over the lanes seeded with the
//           saved carry (the release step of slot E, the running maximum of
//           T[0 .. E - 1]); order[k] = t | FX_ORDER_SCC_START, release[t] =
//           the maximum; stop at the first absent slot.
//   pass C  the rows of [done, f) whose slot is above the new E get
//           FX_RELEASE_NONE.  Pass B stores the release of rows whose slot is
//           at most the new E, pass C of rows whose slot is above it: no
//           address is stored by two lanes in one launch.
// At commit the rows of [done, f) execute at their own step, only slot 0
// fails, E is the count and T is not used.  Lane 0 writes the header last.
// The rows at or after f have been through pass A, so a stopped stream's T
// holds rows that were never handled; a stopped stream's T is not read again.
//
// The memory rules are k_slot_scan's, for its reasons:
//   T's words are written by one lane (the clear, the min-atomic) and read
//   back by another lane of the same wavefront (the bad-row check, pass B), so
//   every access to T is an agent-scope relaxed atomic (store, min, load),
//   served at the L2 in the order the wavefront issued it: no plain load that
//   could hit a stale L1 line, no fence per element; one wavefront-scope fence
//   between the passes keeps the compiler from moving an access across them.
//   The header is read and written by lane 0 only, with plain vector accesses:
//   it is read before anything of this launch is stored and written after
//   everything else, and no other lane or wavefront touches it in a launch.
//   `order` and `release` are plain vector stores that are never read.  A
//   stream's state belongs to its wavefront alone: nothing is handed from one
//   workgroup to another, there is no barrier and no spin loop.  Every loop is
//   bounded by len or steps, every index into T is checked against steps, and
//   the header is validated (fx::slot_header_ok) before anything of it is used.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fantoch_amd.h"
#include "fx_internal.h"
#include "fx_slot.h"
#include "fx_wave.h"

namespace {

struct AArgs {
  fx_slot_batch in;
  fx_order_batch out;
  uint32_t* state;
  uint32_t at_commit, init;
};

using fx::ctz64;
using fx::rl;

__device__ __forceinline__ uint32_t t_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(64) void k_slot_advance(const AArgs a) {
  const uint32_t s = fx::xcd_slot(blockIdx.x), lane = threadIdx.x, steps = a.in.steps;
  if (s >= a.in.num_streams) return;
  const uint32_t len = fx::slot_length(a.in.lengths, s, steps);
  const uint32_t* const slot = a.in.slot;
  uint32_t* const H = a.state + (size_t)s * fx::slot_session_stride(steps);
  uint32_t* const T = H + fx::SLOT_H_WORDS;  // T[slot - 1]
  uint32_t done = 0u, E = 0u, carry = 0u, status = FX_OK;

  if (a.init) {
    for (uint32_t i = lane; i < steps; i += 64u)
      __hip_atomic_store(&T[i], FX_RELEASE_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    uint32_t tag = 0u, hsteps = 0u;
    if (lane == 0) {
      tag = H[fx::SLOT_H_TAG], hsteps = H[fx::SLOT_H_STEPS], done = H[fx::SLOT_H_DONE];
      E = H[fx::SLOT_H_E], carry = H[fx::SLOT_H_CARRY], status = H[fx::SLOT_H_ERR];
    }
    tag = rl(tag, 0), hsteps = rl(hsteps, 0), done = rl(done, 0);
    E = rl(E, 0), carry = rl(carry, 0), status = rl(status, 0);
    if (!fx::slot_header_ok(tag, hsteps, done, E, steps, a.at_commit != 0u)) {
      if (lane == 0) a.out.err[s] = FX_ERR_INVALID_ARG;
      return;
    }
    // a stream that stopped stays stopped; one with no new rows is done
    if (status || len <= done) {
      if (lane == 0) {
        if (!status && len < done) {
          a.out.err[s] = FX_ERR_INVALID_ARG;
        } else {
          a.out.nexec[s] = E;
          a.out.err[s] = status;
        }
      }
      return;
    }
  }

  if (a.at_commit) {
    for (uint32_t r0 = done; r0 < len && !status; r0 += 64u) {
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
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // pass A: the first arrival row of every slot, the rows of earlier calls included
    for (uint32_t r = done + lane; r < len; r += 64u) {
      const uint32_t v = slot[fx_index(r, s, steps)];
      if (v - 1u < steps) __hip_atomic_fetch_min(&T[v - 1u], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // the first bad row and its kind
    uint32_t f = len;
    for (uint32_t r = done + lane; r < len && f == len; r += 64u) {
      const uint32_t v = slot[fx_index(r, s, steps)];
      if (v - 1u >= steps || t_load(&T[v - 1u]) != r) f = r;
    }
    f = fx::wave_min(f);
    if (f < len) {
      const uint32_t v = slot[fx_index(f, s, steps)];
      status = v > steps ? FX_ERR_CAPACITY : FX_ERR_SLOT;
    }
    // pass B: the executed prefix from slot index E on, 64 slots per trip.  At
    // most f slots have executed after this call, so k0 < f bounds the trips.
    for (uint32_t k0 = E; k0 < f; k0 += 64u) {
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
      if (cnt != 0u) carry = rl(m, cnt - 1u);
      if (cnt < 64u) break;
    }
    // pass C: the rows of this call below f whose slot still waits
    for (uint32_t r = done + lane; r < f; r += 64u)
      if (slot[fx_index(r, s, steps)] > E) a.out.release[fx_index(r, s, steps)] = FX_RELEASE_NONE;
  }
  if (lane == 0) {
    H[fx::SLOT_H_TAG] = fx::SLOT_TAG | (a.at_commit ? 1u : 0u);
    H[fx::SLOT_H_STEPS] = steps;
    H[fx::SLOT_H_DONE] = len;
    H[fx::SLOT_H_E] = E;
    H[fx::SLOT_H_CARRY] = carry;
    H[fx::SLOT_H_ERR] = status;
    a.out.nexec[s] = E;
    a.out.err[s] = status;
  }
}

}  // namespace

using namespace fx;

extern "C" int fx_slot_advance(const fx_slot_batch* in, const fx_order_batch* out, void* state, uint32_t flags,
                               void* hip_stream) {
  const int st = slot_advance_check(in, out, state, flags);
  if (st) return st;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (in->num_streams == 0u || in->steps == 0u) return FX_OK;
  if (in->num_streams > 0x7FFFFFC0u) return FX_ERR_INVALID_ARG;
  const AArgs a{*in, *out, (uint32_t*)state, (flags & FX_FLAG_EXECUTE_AT_COMMIT) ? 1u : 0u,
                (flags & FX_FLAG_INIT) ? 1u : 0u};
  hipLaunchKernelGGL(k_slot_advance, dim3(xcd_grid(in->num_streams)), dim3(64), 0, (hipStream_t)hip_stream, a);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}
