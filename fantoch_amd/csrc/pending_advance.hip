// pending_advance.hip — resumable streams of the pending stage
// (fx_pending_advance): k_pending<true>'s chunk step (pending_exec.hip, kept
// here as a copy: that file stays as it is) continued from a saved table.  The
// semantics: fantoch_amd.h; the state layout, the argument check and the
// header check, shared with the host twin (pending_host.cpp): fx_pending.h.
//
// k_pending_advance: a wavefront per stream and workgroup, 64 order rows per
// iteration, lane i holding row k0 + i, k0 = done, done + 64, ...  Per stream
// the state is a header {tag, steps, count_mask, process, done, nready, live,
// err} and the HBM tier's table: pending_buckets(steps) buckets of 64 entries
// of 16 bytes, the bucket function and the owner-lane rule of k_pending<true>
// (entry i of every bucket is read and written by lane i only, so a lane only
// ever reads back its own stores, in program order).  FX_FLAG_INIT clears the
// table, no later call does: the builders that are live at the end of a call
// stay in it.  The chunk step is k_pending's: count-1 rows complete at once;
// for every distinct rifl of the other rows the builder is looked up once, a
// lane's place in the run gives its command, its slot and its head row; the
// first failing row stops the stream and nothing of the lanes from it on is
// stored; the builders that outlive the chunk enter the table.
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
// count and its head row are in range, so no index comes from memory
// unchecked.  No barrier, no spin loop, no atomic; every store is a plain
// vector store; lanes tell each other things through ballot, readlane and
// shuffles only.  Every loop is bounded by nexec, steps or buckets.
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

using fx::ctz64;
using fx::pop64;
using fx::rl;

__global__ __launch_bounds__(64) void k_pending_advance(const PaArgs a) {
  const uint32_t s = fx::xcd_slot(blockIdx.x), lane = threadIdx.x;
  if (s >= a.in.num_streams) return;
  const uint32_t steps = a.in.steps, ne = a.in.nexec[s], buckets = a.buckets;
  uint32_t* const H = a.state + (size_t)s * fx::pending_session_stride(steps);
  uint4* const tab = (uint4*)(H + fx::PENDING_H_WORDS);
  uint32_t done = 0u, nready = 0u, live = 0u, status = FX_OK;

  if (a.init) {
    for (uint32_t i = lane; i < buckets * 64u; i += 64u) tab[i] = make_uint4(0u, 0u, 0u, 0u);
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

  for (uint32_t k0 = done; k0 < end; k0 += 64u) {
    const uint32_t k = k0 + lane;
    uint32_t arow = 0u, r = 0u, c = 0u;
    bool sbad = false;
    if (k < end) {
      arow = FX_ORDER_REC(a.in.order[fx_index(k, s, steps)]);
      if (arow >= steps) {
        sbad = true;
      } else {
        const size_t at = fx_index(arow, s, steps);
        r = a.in.rifl[at];
        c = fx::pending_count(a.in.count[at], a.in.count_mask, r, a.in.process);
        sbad = c > FX_PENDING_MAX_PARTS;
      }
    }
    const uint64_t sfail = __ballot(sbad);
    const bool act = k < end && (sfail == 0ull || lane < ctz64(sfail));
    const bool multi = act && c > 1u;
    uint32_t head = arow, slot = 0u, ins_w = 0u;
    bool creates = false, completes = act && c == 1u, inserts = false;
    uint64_t mfail = 0ull;

    uint64_t un = __ballot(multi);
    while (un) {
      const uint32_t first = ctz64(un);
      const uint32_t rr = rl(r, first);
      uint64_t m = __ballot(multi && r == rr) & un;
      // the builder of rr
      bool found = false;
      uint32_t loc = 0u, bw = 0u, bhead = 0u;
      uint32_t bk = fx::pending_bucket(rr, buckets);
      for (uint32_t probe = 0; probe < buckets; ++probe) {
        const uint4 e = tab[bk * 64u + lane];
        // a live entry of rr whose count and head row are what a session writes
        const uint64_t hit = __ballot((e.z & fx::PENDING_LIVE) != 0u && e.x == rr && e.y < steps &&
                                      fx::pending_word_count(e.z) - 2u <= FX_PENDING_MAX_PARTS - 2u);
        if (hit) {
          const uint32_t l = ctz64(hit);
          found = true;
          loc = bk * 64u + l;
          bw = rl(e.z, l);
          bhead = rl(e.y, l);
          break;
        }
        if (__ballot(e.z == 0u)) break;
        bk = bk + 1u == buckets ? 0u : bk + 1u;
      }
      const uint32_t g0 = found ? fx::pending_word_got(bw) : 0u;
      const uint32_t C = found ? fx::pending_word_count(bw) : rl(c, first);
      const uint64_t other = m & __ballot(c != C);
      if (other) {  // the run ends before the first lane of another count
        const uint32_t L = ctz64(other);
        const uint64_t run = m & ((1ull << L) - 1ull);
        if ((g0 + pop64(run)) % C != 0u) {  // a builder of count C is live at lane L
          mfail |= 1ull << L;
          un &= ~m;
        }
        m = run;
      }
      un &= ~m;
      const uint32_t total = g0 + pop64(m);
      const bool mine = (m >> lane) & 1ull;
      const uint32_t p = g0 + pop64(m & below);
      uint32_t q = 0u, sl = p, rem = total == C ? 0u : total;
      if (total > C) {
        q = p / C;
        sl = p - q * C;
        rem = total % C;
      }
      const bool cr = mine && sl == 0u;
      const uint64_t crs = __ballot(cr) & (below | (1ull << lane));
      // every lane takes part in the exchange
      const uint32_t from = (uint32_t)__shfl((int)arow, (int)(crs ? 63u - (uint32_t)__builtin_clzll(crs) : lane));
      if (mine) {
        head = crs ? from : bhead;
        slot = sl;
        creates = cr;
        completes = sl == C - 1u;
        // the builder created in this chunk that outlives it
        if (rem != 0u && (!found || total > C) && p == total - rem) {
          inserts = true;
          ins_w = fx::pending_word(C, rem);
        }
      }
      if (found) {
        const uint32_t w = total >= C ? fx::PENDING_DONE : fx::pending_word(C, total);
        if (lane == (loc & 63u)) tab[loc] = make_uint4(rr, bhead, w, 0u);
      }
    }

    const uint64_t crs = __ballot(creates), cps = __ballot(completes && c > 1u), fin = __ballot(completes);
    const uint64_t fail = sfail | mfail;
    const uint64_t ok = fail ? (1ull << ctz64(fail)) - 1ull : ~0ull;
    if (act && ((ok >> lane) & 1ull)) {
      const size_t at = fx_index(arow, s, steps);
      if (c == 0u) {
        a.out.head[at] = FX_PENDING_IGNORED;
      } else {
        const size_t hat = fx_index(head, s, steps);
        a.out.part[slot * a.plane + hat] = arow;
        a.out.head[at] = head;
        if (completes) {
          const uint32_t i = nready + pop64(fin & below);
          a.out.index[hat] = i;
          a.out.ready[fx_index(i, s, steps)] = head;
        }
      }
    }
    nready += pop64(fin & ok);
    live += pop64(crs & ok) - pop64(cps & ok);
    if (fail) {
      status = FX_ERR_INVALID_ARG;
      break;
    }

    uint64_t ins = __ballot(inserts);
    while (ins) {
      const uint32_t l = ctz64(ins);
      ins &= ins - 1ull;
      const uint32_t ir = rl(r, l), ih = rl(arow, l), iw = rl(ins_w, l);
      uint32_t bk = fx::pending_bucket(ir, buckets);
      for (uint32_t probe = 0; probe < buckets; ++probe) {
        const uint4 e = tab[bk * 64u + lane];
        const uint64_t unused = __ballot(e.z == 0u);
        if (unused) {
          if (lane == ctz64(unused)) tab[bk * 64u + lane] = make_uint4(ir, ih, iw, 0u);
          break;
        }
        bk = bk + 1u == buckets ? 0u : bk + 1u;
      }
    }
  }

  if (lane == 0) {
    H[fx::PENDING_H_TAG] = fx::PENDING_TAG, H[fx::PENDING_H_STEPS] = steps;
    H[fx::PENDING_H_MASK] = a.in.count_mask, H[fx::PENDING_H_PROCESS] = a.in.process;
    H[fx::PENDING_H_DONE] = end, H[fx::PENDING_H_NREADY] = nready, H[fx::PENDING_H_LIVE] = live;
    H[fx::PENDING_H_ERR] = status;
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
