// pending_advance.hip — resumable streams of the pending stage
// (fx_pending_advance): k_pending<true>'s chunk step continued from a saved
// table.  The chunk step and the table are stated once, in pending_step.inc,
// for this kernel and k_pending (pending_exec.hip).  The semantics:
// fantoch_amd.h; the state layout, the argument check, the header check and
// the header write, shared with the host twin (pending_host.cpp): fx_pending.h.
//
// k_pending_advance: a wavefront per stream and workgroup, 64 order rows per
// iteration, lane i holding row k0 + i, k0 = done, done + 64, ...  Per stream
// the state is a header {tag, steps, count_mask, process, done, nready, live,
// err} and the HBM tier's table: pending_buckets(steps) buckets of 64 entries
// of 16 bytes.  FX_FLAG_INIT clears the table, no later call does: the
// builders that are live at the end of a call stay in it.
//
// Why the table does not fill.  A chunk now starts at done, not at a multiple
// of 64, so which builders take an entry differs from a whole run's: a
// builder takes one when it is live at the end of the chunk that created it,
// and the chunks are cut elsewhere.  The capacity argument does not depend on
// where they are cut: an entry is taken by the creating order row of a
// builder, at most once per such row (one insert per creator lane and chunk),
// and entries are never reused (a completed one holds PENDING_DONE).  A stream
// has at most `steps` order rows, so at most `steps` entries are ever taken,
// and the table holds ceil(max(steps, 1) / 64) x 64 >= steps of them: the
// cyclic walk from a rifl's bucket always meets an entry never used, and no
// stream ends with FX_ERR_CAPACITY.  The walk is bounded by `buckets` all the
// same.
//
// The memory rules: the header is read by lane 0 before anything of the
// launch is stored, validated (fx::pending_header_ok) before anything of it
// is used, and written by lane 0 last.  A looked-up entry counts only if its
// count and its head row are in range (PendingBuckets<true>), so no index
// comes from memory unchecked.  No barrier, no spin loop, no atomic; every
// store is a plain vector store; lanes tell each other things through ballot,
// readlane and shuffles only.  Every loop is bounded by nexec, steps or
// buckets.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fantoch_amd.h"
#include "fx_internal.h"
#include "fx_pending.h"
#include "fx_wave.h"

namespace {

struct PaArgs {
  fx_pending_batch in;
  fx_pending_out out;
  size_t plane;
  uint32_t* state;
  uint32_t buckets, init;
};

using fx::rl;

#include "pending_step.inc"

__global__ __launch_bounds__(64) void k_pending_advance(const PaArgs a) {
  const uint32_t s = fx::xcd_slot(blockIdx.x), lane = threadIdx.x;
  if (s >= a.in.num_streams) return;
  const uint32_t steps = a.in.steps, ne = a.in.nexec[s], buckets = a.buckets;
  uint32_t* const H = a.state + (size_t)s * fx::pending_session_stride(steps);
  uint4* const entries = (uint4*)(H + fx::PENDING_H_WORDS);
  uint32_t done = 0u, nready = 0u, live = 0u, status = FX_OK;

  if (a.init) {
    for (uint32_t i = lane; i < buckets * 64u; i += 64u) entries[i] = make_uint4(0u, 0u, 0u, 0u);
  } else {
    uint32_t h[8];
#pragma unroll
    for (uint32_t i = 0; i < 8u; ++i) {
      uint32_t w = 0u;
      if (lane == 0) w = H[i];
      h[i] = rl(w, 0);
    }
    if (!fx::pending_header_ok(h, steps, a.in.count_mask, a.in.process)) {
      if (lane == 0) a.out.err[s] = FX_ERR_INVALID_ARG;
      return;
    }
    done = h[fx::PENDING_H_DONE], nready = h[fx::PENDING_H_NREADY], live = h[fx::PENDING_H_LIVE];
    status = h[fx::PENDING_H_ERR];
    // a stream that stopped stays stopped; one with no new rows is done
    if (status || ne > steps || ne <= done) {
      if (lane == 0)
        a.out.err[s] = status ? status : ne > steps ? FX_ERR_ORDER_OVERFLOW : ne < done ? FX_ERR_INVALID_ARG : FX_OK;
      return;
    }
  }
  // (with FX_FLAG_INIT) nexec > steps: no rows, as the whole stage
  const uint32_t end = ne > steps ? 0u : ne;
  const uint64_t below = (1ull << lane) - 1ull;
  PendingBuckets<true> tab{entries, buckets, steps};

  for (uint32_t k0 = done; k0 < end; k0 += 64u)
    if (!pending_chunk(a.in, a.out, a.plane, s, k0, end, lane, below, tab, nready, live, status)) break;

  if (lane == 0) {
    fx::pending_write_header(H, steps, a.in.count_mask, a.in.process, end, nready, live, status);
    a.out.nready[s] = nready;
    a.out.nopen[s] = live;
    a.out.err[s] = ne > steps ? FX_ERR_ORDER_OVERFLOW : status;
  }
}

}  // namespace

using namespace fx;

extern "C" int fx_pending_advance(const fx_pending_batch* in, const fx_pending_out* out, void* state, uint32_t flags,
                                  void* hip_stream) {
  const int st = pending_advance_check(in, out, state, flags);
  if (st) return st;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (in->num_streams == 0) return FX_OK;
  if (in->num_streams > 0x7FFFFFC0u) return FX_ERR_INVALID_ARG;
  const PaArgs a{*in, *out, fx_plane_words(in->num_streams, in->steps), (uint32_t*)state, pending_buckets(in->steps),
                 (flags & FX_FLAG_INIT) ? 1u : 0u};
  hipLaunchKernelGGL(k_pending_advance, dim3(xcd_grid(in->num_streams)), dim3(64), 0, (hipStream_t)hip_stream, a);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}
