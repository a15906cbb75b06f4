// pending_exec.hip — AggregatePending for a batch (fx_pending_aggregate,
// fx_pending_run): a command's partials collected per rifl, one result row when
// the last has executed.  The semantics: fantoch_amd.h; what is shared with the
// host twin (pending_host.cpp): fx_pending.h.
//
// k_pending: one wavefront per stream and workgroup, 64 order rows per
// iteration, lane i holding row k0 + i: its arrival row, then the rifl and the
// count at that row.  The live builders of the stream sit in registers (ONCHIP:
// lane b = builder b: rifl, head row, state word; a look-up is one compare and
// a ballot) or in the caller's state (HBM: buckets of 64 entries of 16 bytes,
// entry i of every bucket read and written by lane i only, so a lane only ever
// reads back its own stores, in program order, and what the lanes tell each
// other goes through registers: no barrier, no atomic, every store a plain
// vector store; a look-up is one 1 KiB load and a ballot per bucket walked).
//
// Per chunk:
//   rows of count 1   complete at once, their own head; they never see a table
//   the other rows    for every distinct rifl r (the first unserved lane's): m =
//                     ballot(rifl == r), the builder looked up once; a lane's
//                     place is the builder's got + popcount(m below it), which
//                     div / mod the count gives the command of the run it
//                     belongs to and its slot there: slot 0 creates a builder,
//                     slot count - 1 completes one, and a lane's head row is the
//                     arrival row of the nearest creator at or below it in m,
//                     else the looked-up builder's.  The looked-up builder gets
//                     its new got, or is removed, at once; a builder that is
//                     created in the chunk and still live at its end is noted
//                     in its creator's lane.  A lane whose count differs from
//                     the run's ends the run: a builder live there is the
//                     stream's count mismatch, else the lanes from it on are a
//                     run of their own, with a look-up of their own.
//   the first failing row   the lowest lane of: arrival row or count out of
//                     range, a count mismatch, (ONCHIP) a creator that finds
//                     FX_PENDING_ONCHIP_LIVE builders live (the count before the
//                     chunk + creators below - completers below).  Nothing of
//                     the lanes from it on is stored or counted.
//   stores            part / head of every lane below it, index / ready of the
//                     completers (ready row: nready + completers below)
//   inserts           if no row failed, the noted builders enter the table, so
//                     at no time does it hold more than the live builders at
//                     the end of a chunk
#include <hip/hip_runtime.h>
#include <stdint.h>

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

using fx::ctz64;
using fx::pop64;
using fx::rl;

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
  uint4* const tab = HBM ? a.state + (size_t)blk * buckets * 64u : nullptr;
  if (HBM)
    for (uint32_t i = lane; i < buckets * 64u; i += 64u) tab[i] = make_uint4(0u, 0u, 0u, 0u);
  uint32_t t_rifl = 0u, t_head = 0u, t_w = 0u;  // ONCHIP: builder `lane` (t_w 0: free)
  uint32_t nready = 0u, live = 0u, status = FX_OK;
  const uint64_t below = (1ull << lane) - 1ull;

  for (uint32_t k0 = 0; k0 < ne; k0 += 64u) {
    const uint32_t k = k0 + lane;
    uint32_t arow = 0u, r = 0u, c = 0u;
    bool sbad = false;
    if (k < ne) {
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
    const bool act = k < ne && (sfail == 0ull || lane < ctz64(sfail));
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
      if (HBM) {
        uint32_t bk = fx::pending_bucket(rr, buckets);
        for (uint32_t probe = 0; probe < buckets; ++probe) {
          const uint4 e = tab[bk * 64u + lane];
          const uint64_t hit = __ballot((e.z & fx::PENDING_LIVE) != 0u && e.x == rr);
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
      } else {
        const uint64_t hit = __ballot(t_w != 0u && t_rifl == rr);
        if (hit) {
          found = true;
          loc = ctz64(hit);
          bw = rl(t_w, loc);
          bhead = rl(t_head, loc);
        }
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
        const uint32_t w = total >= C ? (HBM ? fx::PENDING_DONE : 0u) : fx::pending_word(C, total);
        if (HBM) {
          if (lane == (loc & 63u)) tab[loc] = make_uint4(rr, bhead, w, 0u);
        } else if (lane == loc) {
          t_w = w;
        }
      }
    }

    const uint64_t crs = __ballot(creates), cps = __ballot(completes && c > 1u), done = __ballot(completes);
    uint64_t cfail = 0ull;
    if (!HBM) cfail = __ballot(creates && live + pop64(crs & below) - pop64(cps & below) >= FX_PENDING_ONCHIP_LIVE);
    const uint64_t fail = sfail | mfail | cfail;
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
          const uint32_t i = nready + pop64(done & below);
          a.out.index[hat] = i;
          a.out.ready[fx_index(i, s, steps)] = head;
        }
      }
    }
    nready += pop64(done & ok);
    live += pop64(crs & ok) - pop64(cps & ok);
    if (fail) {
      status = (cfail >> ctz64(fail)) & 1ull ? FX_ERR_CAPACITY : FX_ERR_INVALID_ARG;
      break;
    }

    uint64_t ins = __ballot(inserts);
    while (ins) {
      const uint32_t l = ctz64(ins);
      ins &= ins - 1ull;
      const uint32_t ir = rl(r, l), ih = rl(arow, l), iw = rl(ins_w, l);
      if (HBM) {
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
      } else {
        const uint64_t vacant = ~__ballot(t_w != 0u);
        if (!vacant) break;  // not reached: live <= FX_PENDING_ONCHIP_LIVE after a chunk that did not fail
        if (lane == ctz64(vacant)) {
          t_rifl = ir;
          t_head = ih;
          t_w = iw;
        }
      }
    }
  }

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
