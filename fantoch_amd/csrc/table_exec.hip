// table_exec.hip — Tempo's TableExecutor on the GPU: one wavefront per stream
// of TableExecutionInfo values, many streams per launch
// (fantoch_ps/src/executor/table/{mod,executor}.rs; shard_count = 1 but for
// the SHARDS kernels below).
//
// Each key owns a VotesTable (mod.rs:104-267).  Here:
//   votes clock   lane v < 16 owns voter v + 1 of every key: its frontier (the
//                 highest c with every vote 1..c seen, the ARClock of
//                 mod.rs:112,127-128) and the votes seen above it live in
//                 column v of the stream's table (LDS or HBM), row = key.  A
//                 lane only ever touches its own column, so the table needs no
//                 cross-lane ordering; an event is one load and one store of
//                 the key's row, and add_range (mod.rs:180) is lane-local
//                 VALU work of the one lane whose voter matches
//   stable clock  element n - stability_threshold of the sorted frontiers
//                 (mod.rs:243-266) = the frontier whose rank, counted by
//                 compares against the n lanes' frontiers, is that index
//   pending ops   (key, clock, dot, arrival) in registers, R per lane
//                 (mod.rs:151-165); stable_ops (mod.rs:196-240) is one ballot
//                 of `key == k && clock <= stable` per register row, each
//                 selected op's position the count of selected ops with a
//                 smaller (clock, dot)
// The stable clock is computed only when the event's key has a pending op
// (and once per key at the end, for the stable_clock output).
//
// ONCHIP tier: the window above a frontier is one word relative to it (bit i
// = vote frontier + 1 + i), R = 1.  HBM tier: a ring bitmap of
// FX_TABLE_HBM_WINDOW bits per (key, voter) in `state`, R = 8.  The window
// arithmetic of both is table_window.h; the windows bound the gaps a range may
// leave above a frontier: a range that starts at its voter's frontier only
// moves it, whatever its length (the single-key ONCHIP kernel alone still
// hands such a range beyond its window to the HBM tier).
//
// MULTI (fx_table_execute_mk): multi-key commands and the StableAtShard
// messages the executor sends itself (executor.rs:168-359, the drain of
// fantoch/src/sim/runner.rs:405-419).  An op keeps its registers after it
// leaves the votes table, until it executes, and gains a meta word:
//   state   in the votes table / queued on its key, untried / tried and
//           counted in the command's stable count / told (the command is
//           stable at the shard and a StableAtShard for this key is on its way)
//   seq     its place in the key's FIFO (PendingPerKey::pending, :33-37): a
//           stream-wide counter taken when the op is queued.  A key's queue
//           head is the op with the lowest seq among the key's queued ops; an
//           op that tried and was handed back is always the head, so it keeps
//           its seq (push_front, :214)
//   nkeys   shard_key_count
// rifl_to_stable_count of a command is the number of its ops in state tried
// (all of them are live registers); when it reaches nkeys those ops' keys are
// the other keys of the command.  to_executors is a ring of (key, dot) held
// one entry per lane and register row (it cannot outgrow the live ops: every
// message on it belongs to a told op), stable_shards_buffered a table of
// (key, dot, count), one entry per lane.
//
// SHARDS (fx_table_execute_ps, with MULTI): commands that span shards.  An op
// gains a second word, missing_stable_shards | shards << 8 (Pending, :40-76):
// a try that makes the command stable at this shard (its only key here, :311-316,
// or the last of its keys here, :328-341) takes one off, stores the step into
// the stable_sent plane and leaves the op told; buffered counts are taken off
// when the op is tried (:345-347) and the op executes at 0.  A StableAtShard
// event from another shard goes through stable_msg like a popped message
// (:168-235): one off the head's count, the head executes at 0.
// On the HBM tier stable_shards_buffered moves into `state`, behind the
// stream's votes tables: FX_TABLE_PS_HBM_BUFFERED entries of (key, dot, count),
// entry e owned by lane e & 63, so like the votes tables it needs no cross-lane
// ordering; only the rows in use are searched.
//
// RESUME (fx_table_advance; HBM tier, one kernel per kind): a stream is fed in
// pieces.  What the wavefront holds in registers -- the pending ops and their
// meta words, the to_executors ring, the counters -- is stored behind the
// stream's tables in `state` when a call ends and loaded when the next begins
// (table_state.h), so for any partition of a stream into calls the outputs
// are those of one whole-stream call.  A call ends with the drain of its last
// event; what that drain pushed stays on the ring for the drain after the
// next call's first event.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fantoch_amd.h"
#include "fx_internal.h"
#include "table_state.h"
#include "table_window.h"

namespace fx {
namespace table {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t NV = 16;                           // voter columns
constexpr uint32_t WB = FX_TABLE_HBM_WINDOW / 32u;    // HBM window words per (key, voter)
constexpr uint32_t ONCHIP_WPB = 4;                    // streams per workgroup, ONCHIP tier
constexpr uint32_t HBM_R = FX_TABLE_HBM_PENDING / 64u;

struct TArgs {
  const uint32_t* hdr;
  const uint32_t* dot;
  const uint32_t* clock;
  const uint32_t* votes;
  const uint32_t* lengths;
  uint32_t S, steps, n, keys, vmax, thr;
  size_t plane;
  uint32_t* order;
  uint32_t* release;
  uint32_t* nexec;
  uint32_t* err;
  uint32_t* stable;
  const uint32_t* stream_map;
  uint32_t num_lanes;
  uint32_t* state;
  uint32_t flags;
  const uint32_t* nkeys;  // MULTI only
  uint32_t* sent;         // SHARDS only: the stable_sent plane, or null
};

// HBM table of one stream: row j, column v at [j * NV + v]; rows 0..keys-1
// the frontiers, row keys + k * WB + i word i of key k's windows
__host__ __device__ constexpr inline size_t hbm_words(uint32_t keys) { return (size_t)keys * NV * (1u + WB); }
static_assert(TS_NV == NV && TS_WB == WB && ts_votes_words(999) == hbm_words(999), "table_state.h describes these tables");

__device__ __forceinline__ uint32_t rl(uint32_t v, uint32_t lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}

// MULTI: an op's meta word = seq (26 bits: steps < 2^26) | state << 26 | (nkeys - 1) << 28
constexpr uint32_t SEQ_MASK = (1u << 26) - 1u;
constexpr uint32_t ST_TABLE = 0, ST_QUEUED = 1, ST_TRIED = 2, ST_TOLD = 3;
__device__ __forceinline__ uint32_t m_state(uint32_t m) { return (m >> 26) & 3u; }
__device__ __forceinline__ uint32_t m_nkeys(uint32_t m) { return (m >> 28) + 1u; }
__device__ __forceinline__ uint32_t m_with(uint32_t m, uint32_t state) { return (m & ~(3u << 26)) | (state << 26); }

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

// the frontier at index n - thr of the n frontiers (lanes 0..n-1) sorted
// ascending: ties broken by lane, so exactly one lane has that rank
__device__ __forceinline__ uint32_t stable_of(uint32_t f, uint32_t n, uint32_t thr, uint32_t lid) {
  uint32_t rank = 0;
  for (uint32_t j = 0; j < n; ++j) {
    const uint32_t fj = rl(f, j);
    rank += (fj < f || (fj == f && j < lid)) ? 1u : 0u;
  }
  const uint64_t b = __ballot(lid < n && rank == n - thr);
  return rl(f, (uint32_t)__builtin_ctzll(b));
}

// RESUME (fx_table_advance, HBM only): the stream starts at the row its last
// call stopped at, with the registers below loaded from the image behind its
// tables in `state` (table_state.h), and stores them back at the end; the
// tables are zeroed with FX_FLAG_INIT only.
template <bool HBM, uint32_t R, uint32_t WPB, bool MULTI, bool SHARDS = false, bool RESUME = false>
__global__ __launch_bounds__(64 * WPB) void k_table(TArgs a) {
  static_assert(!RESUME || (HBM && R == TS_R && WPB == 1), "resumable streams keep their tables in `state`");
  constexpr uint32_t KIND = SHARDS ? FX_TABLE_KIND_PS : MULTI ? FX_TABLE_KIND_MK : FX_TABLE_KIND_SINGLE;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const uint32_t wv = WPB > 1 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0u;
  const uint32_t li = xcd_slot(blockIdx.x) * WPB + wv;
  if (li >= a.num_lanes) return;  // whole wavefront
  const uint32_t lid = threadIdx.x & 63u;
  const uint32_t s = a.stream_map ? a.stream_map[li] : li;
  const uint32_t n = a.n, keys = a.keys;
  const bool vlane = lid < NV;
  const bool at_commit = (a.flags & FX_FLAG_EXECUTE_AT_COMMIT) != 0;
  constexpr bool BMEM = HBM && SHARDS;  // stable_shards_buffered in `state`
  constexpr uint32_t BN = FX_TABLE_PS_HBM_BUFFERED, BROWS = BN / 64u;
  uint32_t* const g = !HBM ? nullptr
                      : RESUME ? a.state + (size_t)li * ts_stride(KIND, keys)
                               : a.state + (size_t)li * (hbm_words(keys) + (BMEM ? 3u * BN : 0u));
  // [e] key, [BN + e] dot, [2 * BN + e] count (0 = free) of entry e = row * 64 + lane
  uint32_t* const gb = BMEM ? g + hbm_words(keys) : nullptr;
  (void)gb;
  uint32_t* const img = RESUME ? g + ts_image_at(KIND, keys) : nullptr;
  (void)img;
  const bool init = !RESUME || (a.flags & FX_FLAG_INIT) != 0;
  uint32_t hv = 0;  // RESUME: the header words, word w on lane w
  (void)hv;
  if constexpr (RESUME) {
    if (!init) {
      const uint32_t len = a.lengths ? min(a.lengths[s], a.steps) : a.steps;
      hv = img[ts_hdr(lid)];
      // the session contract; then a stream that stopped stays stopped, and one
      // with no new rows is done: nothing but err and nexec is written
      const bool same = rl(hv, TS_H_STEPS) == a.steps && rl(hv, TS_H_N) == n && rl(hv, TS_H_KEYS) == keys &&
                        rl(hv, TS_H_VMAX) == a.vmax && rl(hv, TS_H_THR) == a.thr && rl(hv, TS_H_KIND) == KIND &&
                        rl(hv, TS_H_AT_COMMIT) == (at_commit ? 1u : 0u);
      const uint32_t was = same ? rl(hv, TS_H_ERR) : (uint32_t)FX_ERR_INVALID_ARG;
      const uint32_t dn = rl(hv, TS_H_DONE);
      if (was || len <= dn) {
        if (lid == 0) {
          a.nexec[s] = rl(hv, TS_H_NEXEC);
          a.err[s] = was ? was : len < dn ? (uint32_t)FX_ERR_INVALID_ARG : 0u;
        }
        return;
      }
    }
  }
  if constexpr (BMEM)
    if (init)
      for (uint32_t j = 0; j < BROWS; ++j) gb[2u * BN + j * 64u + lid] = 0;
  // ONCHIP: key k's row = 32 words, [lb + k * 32 + v] frontier, [+ 16 + v] window
  const uint32_t lb = wv * keys * 32u;
  if (vlane && init) {
    if constexpr (HBM) {
      for (size_t j = 0; j < (size_t)keys * (1u + WB); ++j) g[j * NV + lid] = 0;
    } else {
      for (uint32_t k = 0; k < keys; ++k) {
        smem[lb + k * 32u + lid] = 0;
        smem[lb + k * 32u + 16u + lid] = 0;
      }
    }
  }
  uint32_t pk[R], pc[R], pd[R], pa[R];
#pragma unroll
  for (uint32_t i = 0; i < R; ++i) pk[i] = NONE, pc[i] = 0, pd[i] = 0, pa[i] = 0;
  uint32_t nexec = 0, err = 0;
  const uint32_t len = a.lengths ? min(a.lengths[s], a.steps) : a.steps;

  // ---- MULTI: queues, stable counts, to_executors, stable_shards_buffered
  constexpr uint32_t SC = 64u * R;  // ring entries: entry e at lane e & 63, row (e >> 6) % R
  uint32_t pm[R], sk[R], sd[R];     // op meta; ring of (key, dot)
#pragma unroll
  for (uint32_t i = 0; i < R; ++i) pm[i] = 0, sk[i] = 0, sd[i] = 0;
  uint32_t bk = 0, bd = 0, bc = 0;  // one buffered (key, dot, count) per lane, free while bc == 0
  uint32_t bhi = 0;                 // BMEM: rows of the table in `state` that were ever used
  (void)bhi;
  uint32_t pz[R];  // SHARDS: missing_stable_shards | shards << 8
#pragma unroll
  for (uint32_t i = 0; i < R; ++i) pz[i] = 0;
  uint32_t qseq = 0, mb = 0, mt = 0, nbuf = 0, step = 0;  // messages [mb, mt) are on to_executors
  uint32_t start = 0;  // the first row of this call
  if constexpr (RESUME) {
    if (!init) {
      start = rl(hv, TS_H_DONE);
      nexec = rl(hv, TS_H_NEXEC);
#pragma unroll
      for (uint32_t i = 0; i < R; ++i) {
        pk[i] = img[ts_reg(TS_P_KEY, i, lid)], pc[i] = img[ts_reg(TS_P_CLOCK, i, lid)];
        pd[i] = img[ts_reg(TS_P_DOT, i, lid)], pa[i] = img[ts_reg(TS_P_ARRIVAL, i, lid)];
        if constexpr (MULTI) {
          pm[i] = img[ts_reg(TS_P_META, i, lid)];
          sk[i] = img[ts_reg(TS_P_RING_KEY, i, lid)], sd[i] = img[ts_reg(TS_P_RING_DOT, i, lid)];
        }
        if constexpr (SHARDS) pz[i] = img[ts_reg(TS_P_SHARDS, i, lid)];
      }
      if constexpr (MULTI) {
        qseq = rl(hv, TS_H_QSEQ), mb = rl(hv, TS_H_MB), mt = rl(hv, TS_H_MT), nbuf = rl(hv, TS_H_NBUF);
        if constexpr (SHARDS) bhi = rl(hv, TS_H_BHI);
        else bk = img[ts_buf(0, lid)], bd = img[ts_buf(1, lid)], bc = img[ts_buf(2, lid)];
      }
    }
  }

  // do_execute (executor.rs:365-380) of the one op selected by hit[]; SHARDS:
  // ha is its event row, wave-uniform, so one lane stores and the addresses
  // are scalar work (R address pairs per call site cost the HBM kernel its
  // second wave per SIMD)
  auto execute_hit = [&](const bool (&hit)[R], uint32_t ha) __attribute__((always_inline)) {
    if constexpr (SHARDS) {
      if (lid == 0) {
        a.order[fx_index(nexec, s, a.steps)] = ha | FX_ORDER_SCC_START;
        a.release[fx_index(ha, s, a.steps)] = step;
      }
#pragma unroll
      for (uint32_t i = 0; i < R; ++i)
        if (hit[i]) pk[i] = NONE;
    } else {
      (void)ha;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i) {
        if (hit[i]) {
          a.order[fx_index(nexec, s, a.steps)] = pa[i] | FX_ORDER_SCC_START;
          a.release[fx_index(pa[i], s, a.steps)] = step;
          pk[i] = NONE;
        }
      }
    }
    ++nexec;
  };
  // tries the ops of key k's queue from its head until one is handed back
  // (the loops of executor.rs:198-217 and :250-276 around :280-359)
  auto run_queue = [&](uint32_t k) __attribute__((always_inline)) {
    for (;;) {
      uint32_t lo = NONE;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i)
        if (pk[i] == k && m_state(pm[i]) != ST_TABLE) lo = min(lo, pm[i] & SEQ_MASK);
      lo = wave_min(lo);
      if (lo == NONE) return;  // the queue is empty
      bool hit[R];
      uint32_t hm = 0, hd = 0, hz = 0, ha = 0;  // SHARDS: the head's second word and event row
      (void)hz;
      (void)ha;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i) {
        hit[i] = pk[i] == k && m_state(pm[i]) != ST_TABLE && (pm[i] & SEQ_MASK) == lo;
        const uint64_t b = __ballot(hit[i]);
        if (b) hm = rl(pm[i], (uint32_t)__builtin_ctzll(b)), hd = rl(pd[i], (uint32_t)__builtin_ctzll(b));
        if constexpr (SHARDS)
          if (b) hz = rl(pz[i], (uint32_t)__builtin_ctzll(b)), ha = rl(pa[i], (uint32_t)__builtin_ctzll(b));
      }
      if (m_state(hm) != ST_QUEUED) return;  // the head tried before and waits for its StableAtShard
      const uint32_t K = m_nkeys(hm);
      if (K == 1 && (!SHARDS || (hz >> 8) == 1u)) {  // :290-293 (:71-75: one key, one shard)
        execute_hit(hit, ha);
        continue;
      }
      // :319-322: one more op of the command tried (SHARDS with one key here,
      // :311-316: the count is 1 = K at once and there is no other key to tell)
      uint32_t cnt = 0;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i) {
        if (hit[i]) pm[i] = m_with(pm[i], ST_TRIED);
        cnt += (uint32_t)__builtin_popcountll(__ballot(pk[i] != NONE && pd[i] == hd && m_state(pm[i]) == ST_TRIED));
      }
      uint32_t missing = 1;
      bool sends = false;  // this try ran send_stable_msg (:296-309)
      (void)sends;
      if constexpr (SHARDS) missing = hz & 0xFFu;
      if (cnt == K) {  // :328-341: the other keys are told, ascending
        for (uint32_t j = 1; j < K; ++j) {
          uint32_t ok = NONE;
#pragma unroll
          for (uint32_t i = 0; i < R; ++i)
            if (pk[i] != NONE && pk[i] != k && pd[i] == hd && m_state(pm[i]) == ST_TRIED) ok = min(ok, pk[i]);
          ok = wave_min(ok);
          if (ok == NONE) break;  // (nkeys - 1 other ops tried: there is one)
          if (mt - mb >= SC) { err = FX_ERR_CAPACITY; return; }
          const uint32_t e = mt % SC;
#pragma unroll
          for (uint32_t i = 0; i < R; ++i) {
            if (pk[i] == ok && pd[i] == hd && m_state(pm[i]) == ST_TRIED) pm[i] = m_with(pm[i], ST_TOLD);
            if ((e >> 6) == i && lid == (e & 63u)) sk[i] = ok, sd[i] = hd;
          }
          ++mt;
        }
        if constexpr (SHARDS) --missing, sends = true;  // :316, :333
        else missing = 0;
      }
      if (nbuf) {  // :345-347
        if constexpr (BMEM) {
          for (uint32_t j = 0; j < bhi; ++j) {
            const uint32_t o = j * 64u + lid, oc = gb[2u * BN + o];
            const uint64_t b = __ballot(oc != 0 && gb[o] == k && gb[BN + o] == hd);
            if (b) {
              const uint32_t l = (uint32_t)__builtin_ctzll(b), c = rl(oc, l);
              if (c > missing) { err = FX_ERR_INVALID_ARG; return; }  // (before anything of this try is written)
              missing -= c;
              if (lid == l) gb[2u * BN + o] = 0;
              --nbuf;
              break;
            }
          }
        } else {
          const uint64_t b = __ballot(bc != 0 && bk == k && bd == hd);
          if (b) {
            const uint32_t l = (uint32_t)__builtin_ctzll(b);
            if constexpr (SHARDS)
              if (rl(bc, l) > missing) { err = FX_ERR_INVALID_ARG; return; }  // (before anything of this try is written)
            missing -= rl(bc, l);
            if (lid == l) bc = 0;
            --nbuf;
          }
        }
      }
      if constexpr (SHARDS) {
#pragma unroll
        for (uint32_t i = 0; i < R; ++i) {
          if (hit[i]) {
            pz[i] = (pz[i] & ~0xFFu) | missing;
            if (sends) pm[i] = m_with(pm[i], ST_TOLD);
          }
        }
        if (sends && a.sent && lid == 0) a.sent[fx_index(ha, s, a.steps)] = step;
      }
      if (missing != 0) return;  // :353-357: handed back, it stays the head
      execute_hit(hit, ha);      // :349-352
    }
  };
  // handle_stable_msg (executor.rs:168-235)
  auto stable_msg = [&](uint32_t k, uint32_t d) __attribute__((always_inline)) {
    uint32_t lo = NONE;
#pragma unroll
    for (uint32_t i = 0; i < R; ++i)
      if (pk[i] == k && m_state(pm[i]) != ST_TABLE) lo = min(lo, pm[i] & SEQ_MASK);
    lo = wave_min(lo);
    bool hit[R];
    uint64_t any = 0;
#pragma unroll
    for (uint32_t i = 0; i < R; ++i) {
      hit[i] = pk[i] == k && m_state(pm[i]) != ST_TABLE && (pm[i] & SEQ_MASK) == lo && pd[i] == d;
      any |= __ballot(hit[i]);
    }
    if (lo != NONE && any) {  // :173-217: missing_stable_shards 1 -> 0
      uint32_t ha = 0;
      if constexpr (SHARDS) {     // :177-186: one off, the head executes at 0
        uint32_t z = 0;
#pragma unroll
        for (uint32_t i = 0; i < R; ++i) {
          const uint64_t b = __ballot(hit[i]);
          if (b) z = rl(pz[i], (uint32_t)__builtin_ctzll(b)), ha = rl(pa[i], (uint32_t)__builtin_ctzll(b));
        }
        if ((z & 0xFFu) != 1u) {
#pragma unroll
          for (uint32_t i = 0; i < R; ++i)
            if (hit[i]) pz[i] -= 1u;
          return;
        }
      }
      execute_hit(hit, ha);
      run_queue(k);
      return;
    }
    // :219-233
    if constexpr (BMEM) {
      for (uint32_t j = 0; j < bhi; ++j) {
        const uint32_t o = j * 64u + lid, oc = gb[2u * BN + o];
        const uint64_t b = __ballot(oc != 0 && gb[o] == k && gb[BN + o] == d);
        if (b) {
          if (lid == (uint32_t)__builtin_ctzll(b)) gb[2u * BN + o] = oc + 1u;
          return;
        }
      }
      for (uint32_t j = 0; j < BROWS; ++j) {
        const uint32_t o = j * 64u + lid;
        const uint64_t fr = __ballot(gb[2u * BN + o] == 0);
        if (fr) {
          if (lid == (uint32_t)__builtin_ctzll(fr)) gb[o] = k, gb[BN + o] = d, gb[2u * BN + o] = 1;
          bhi = max(bhi, j + 1u);
          ++nbuf;
          return;
        }
      }
      err = FX_ERR_CAPACITY;
      return;
    }
    const uint64_t b = __ballot(bc != 0 && bk == k && bd == d);
    if (b) {
      if (lid == (uint32_t)__builtin_ctzll(b)) ++bc;
      return;
    }
    const uint64_t fr = __ballot(bc == 0);
    if (!fr) { err = FX_ERR_CAPACITY; return; }
    if (lid == (uint32_t)__builtin_ctzll(fr)) bk = k, bd = d, bc = 1;
    ++nbuf;
  };
  // the runner's drain after an event (fantoch/src/sim/runner.rs:411-416): the
  // messages on to_executors now, last pushed first, each handled once; what
  // the handlers push waits for the next event's drain.  It runs before the
  // next event is looked at, and once after the last.
  auto drain = [&]() __attribute__((always_inline)) {
    const uint32_t top = mt;
    for (uint32_t e = top; e != mb && !err;) {
      --e;
      const uint32_t x = e % SC;
      uint32_t mk = 0, md = 0;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i)
        if ((x >> 6) == i) mk = rl(sk[i], x & 63u), md = rl(sd[i], x & 63u);
      stable_msg(mk, md);
    }
    mb = top;
  };

  // the inputs of the 4-step tile row holding step r0: lane 4q + k holds step
  // r0 + k of plane q -- 0 hdr, 1 dot, 2 clock, 3 + p vote plane p (p < 12:
  // the first four vote slots) -- one load, issued a row ahead of its use
  auto row_load = [&](uint32_t r0) -> uint32_t {
    const uint32_t q = lid >> 2;
    const size_t at = fx_index(r0 + (lid & 3u), s, a.steps);
    if (q == 0) return a.hdr[at];
    if (q == 1) return a.dot[at];
    if (q == 2) return a.clock[at];
    const uint32_t p = q - 3u;
    if constexpr (MULTI)
      if (q == 15u) return a.nkeys[at];  // lanes 60..63
    return (q < 15u && p < 3u * a.vmax) ? a.votes[(size_t)p * a.plane + at] : 0u;
  };
  // (a resumed call starts inside a tile row: that row first)
  const uint32_t row0 = start & ~3u;
  uint32_t row = len ? row_load(row0) : 0u, next = len > row0 + 4 ? row_load(row0 + 4) : 0u;

  for (uint32_t r = start; r < len; ++r) {
    if constexpr (MULTI) {
      // of the event before (events that `continue` push nothing).  The call
      // before a resumed one ended with the drain of its last event: what that
      // pushed waits for the drain of this call's first
      if (!RESUME || r != start) drain();
      if (err) break;
      step = r;
    }
    if (r != start && !(r & 3u)) {
      row = next;
      if (r + 4 < len) next = row_load(r + 4);
    }
    const uint32_t kq = r & 3u;
    const size_t at = fx_index(r, s, a.steps);
    const uint32_t h = rl(row, kq);
    const uint32_t k = FX_TABLE_HDR_KEY(h), nv = FX_TABLE_HDR_NVOTES(h);
    if constexpr (SHARDS) {
      if (h >> 24 == FX_TABLE_HDR_STABLE(0) >> 24) {  // StableAtShard from another shard (:140-142)
        if (k >= keys) { err = FX_ERR_INVALID_ARG; break; }
        const uint32_t d = rl(row, 4u + kq);
        if (FX_DOT_SRC(d) < 1 || FX_DOT_SRC(d) > n || FX_DOT_SEQ(d) == 0) { err = FX_ERR_DOT_RANGE; break; }
        if (!at_commit) stable_msg(k, d);
        if (err) break;
        continue;  // (the drain comes before the next event, or after the last)
      }
    }
    if (nv > a.vmax || k >= keys) { err = FX_ERR_INVALID_ARG; break; }
    if (FX_TABLE_HDR_KIND(h) == FX_TABLE_ATTACHED) {
      const uint32_t d = rl(row, 4u + kq), c = rl(row, 8u + kq);
      const uint32_t src = FX_DOT_SRC(d);
      uint32_t K = 1, SH = 1;
      (void)K;
      (void)SH;
      if constexpr (MULTI) {
        K = rl(row, 60u + kq);
        if constexpr (SHARDS) {  // FX_TABLE_PS_WORD(nkeys, shards)
          SH = K >> 8;
          K &= 0xFFu;
          if (SH < 1 || SH > FX_TABLE_MAX_CMD_SHARDS) { err = FX_ERR_INVALID_ARG; break; }
        }
        if (K < 1 || K > FX_TABLE_MAX_CMD_KEYS) { err = FX_ERR_INVALID_ARG; break; }
      }
      if (src < 1 || src > n || FX_DOT_SEQ(d) == 0) { err = FX_ERR_DOT_RANGE; break; }
      if (at_commit) {  // executor.rs:125-126
        if (lid == 0) {
          a.order[fx_index(nexec, s, a.steps)] = r | FX_ORDER_SCC_START;
          a.release[at] = r;
        }
        ++nexec;
        continue;
      }
      // ops.insert(sort_id, pending) must find the slot free (mod.rs:163-165)
      uint64_t dup = 0;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i)
        dup |= __ballot(pk[i] == k && pc[i] == c && pd[i] == d && (!MULTI || m_state(pm[i]) == ST_TABLE));
      if (dup) { err = FX_ERR_DOUBLE_INDEX; break; }
      if constexpr (MULTI) {
        // the input contract, against the command's ops that have not executed:
        // same nkeys (and shards) and clock, another key, fewer than nkeys, none told
        uint64_t bad = 0;
        uint32_t mates = 0;
#pragma unroll
        for (uint32_t i = 0; i < R; ++i) {
          const bool m = pk[i] != NONE && pd[i] == d;
          mates += (uint32_t)__builtin_popcountll(__ballot(m));
          bad |= __ballot(m && (pk[i] == k || pc[i] != c || m_nkeys(pm[i]) != K || m_state(pm[i]) == ST_TOLD ||
                                (SHARDS && (pz[i] >> 8) != SH)));
        }
        if (bad || mates >= K) { err = FX_ERR_INVALID_ARG; break; }
      }
      bool placed = false;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i) {
        if (!placed) {
          const uint64_t fr = __ballot(pk[i] == NONE);
          if (fr) {
            if (lid == (uint32_t)__builtin_ctzll(fr)) {
              pk[i] = k, pc[i] = c, pd[i] = d, pa[i] = r;
              if constexpr (MULTI) pm[i] = (K - 1u) << 28;
              if constexpr (SHARDS) pz[i] = SH | (SH << 8);
            }
            placed = true;
          }
        }
      }
      if (!placed) { err = FX_ERR_CAPACITY; break; }
    } else if (at_commit) {
      continue;  // executor.rs:134-139: votes are ignored
    }

    // add_detached_votes (mod.rs:171-194): the ranges in order, each on the
    // lane of its voter
    uint32_t f = 0, w = 0;
    if (vlane) {
      if constexpr (HBM) {
        f = g[(size_t)k * NV + lid];
      } else {
        f = smem[lb + k * 32u + lid];
        w = smem[lb + k * 32u + 16u + lid];
      }
    }
    uint32_t fail = 0;
    for (uint32_t j = 0; j < nv; ++j) {
      uint32_t voter, st, en;
      if (j < 4u) {
        voter = rl(row, 4u * (3u + 3u * j) + kq);
        st = rl(row, 4u * (4u + 3u * j) + kq);
        en = rl(row, 4u * (5u + 3u * j) + kq);
      } else {
        const uint32_t* vp = a.votes + (size_t)(3u * j) * a.plane + at;
        voter = (uint32_t)__builtin_amdgcn_readfirstlane((int)vp[0]);
        st = (uint32_t)__builtin_amdgcn_readfirstlane((int)vp[a.plane]);
        en = (uint32_t)__builtin_amdgcn_readfirstlane((int)vp[2 * a.plane]);
      }
      if (voter - 1u >= n || st == 0 || st > en) { fail = FX_ERR_VOTE_RANGE; break; }
      uint32_t lf = 0;
      if (lid == voter - 1u) {
        // table_window.h; HBM: word i of this voter's ring at win[i * NV]
        if constexpr (HBM) lf = add_range_ring<!SHARDS>(f, g + ((size_t)keys + (size_t)k * WB) * NV + lid, NV, st, en);
        else lf = add_range_word<MULTI>(f, w, st, en);
      }
      fail = rl(lf, voter - 1u);
      if (fail) break;
    }
    if (fail) { err = fail; break; }
    if (vlane) {
      if constexpr (HBM) {
        g[(size_t)k * NV + lid] = f;
      } else {
        smem[lb + k * 32u + lid] = f;
        smem[lb + k * 32u + 16u + lid] = w;
      }
    }

    // stable_ops (mod.rs:196-240)
    uint64_t onkey = 0;
#pragma unroll
    for (uint32_t i = 0; i < R; ++i) onkey |= __ballot(pk[i] == k && (!MULTI || m_state(pm[i]) == ST_TABLE));
    if (!onkey) continue;
    const uint32_t stable = stable_of(f, n, a.thr, lid);
    bool sel[R];
    uint64_t sb[R];
    uint32_t rank[R], total = 0;
#pragma unroll
    for (uint32_t i = 0; i < R; ++i) {
      sel[i] = pk[i] == k && pc[i] <= stable && (!MULTI || m_state(pm[i]) == ST_TABLE);
      sb[i] = __ballot(sel[i]);
      rank[i] = 0;
      total += (uint32_t)__builtin_popcountll(sb[i]);
    }
    if (!total) continue;
#pragma unroll
    for (uint32_t i2 = 0; i2 < R; ++i2) {
      for (uint64_t b = sb[i2]; b; b &= b - 1u) {
        const uint32_t l = (uint32_t)__builtin_ctzll(b);
        const uint32_t oc = rl(pc[i2], l), od = rl(pd[i2], l);
#pragma unroll
        for (uint32_t i = 0; i < R; ++i) rank[i] += (oc < pc[i] || (oc == pc[i] && od < pd[i])) ? 1u : 0u;
      }
    }
    if constexpr (MULTI) {
      // send_stable_or_execute (executor.rs:237-277).  With the key's queue
      // empty and single-key ops only, all execute at once; otherwise the
      // ops join the queue in their order and, if it was empty, are tried
      // from its head until one is handed back.
      uint64_t queued = 0, multi = 0;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i) {
        queued |= __ballot(pk[i] == k && m_state(pm[i]) != ST_TABLE);
        multi |= __ballot(sel[i] && (m_nkeys(pm[i]) != 1u || (SHARDS && (pz[i] >> 8) != 1u)));
      }
      if (queued || multi) {
#pragma unroll
        for (uint32_t i = 0; i < R; ++i)
          if (sel[i]) pm[i] = (pm[i] & ~(SEQ_MASK | (3u << 26))) | (ST_QUEUED << 26) | (qseq + rank[i]);
        qseq += total;
        if (!queued) run_queue(k);
        continue;
      }
    }
#pragma unroll
    for (uint32_t i = 0; i < R; ++i) {
      if (sel[i]) {
        a.order[fx_index(nexec + rank[i], s, a.steps)] = pa[i] | FX_ORDER_SCC_START;
        a.release[fx_index(pa[i], s, a.steps)] = r;
        pk[i] = NONE;
      }
    }
    nexec += total;
  }
  if constexpr (MULTI)
    if (!err) drain();

  if (a.stable) {
    for (uint32_t k = 0; k < keys; ++k) {
      uint32_t f = 0;
      if (vlane) {
        if constexpr (HBM) f = g[(size_t)k * NV + lid];
        else f = smem[lb + k * 32u + lid];
      }
      const uint32_t sc = stable_of(f, n, a.thr, lid);
      if (lid == 0) a.stable[(size_t)s * keys + k] = sc;
    }
  }
  if (lid == 0) {
    a.nexec[s] = nexec;
    a.err[s] = err;
  }
  if constexpr (RESUME) {
    if (lid == 0) {
      img[ts_hdr(TS_H_STEPS)] = a.steps, img[ts_hdr(TS_H_N)] = n, img[ts_hdr(TS_H_KEYS)] = keys;
      img[ts_hdr(TS_H_VMAX)] = a.vmax, img[ts_hdr(TS_H_THR)] = a.thr, img[ts_hdr(TS_H_KIND)] = KIND;
      img[ts_hdr(TS_H_AT_COMMIT)] = at_commit ? 1u : 0u;
      img[ts_hdr(TS_H_DONE)] = len, img[ts_hdr(TS_H_NEXEC)] = nexec, img[ts_hdr(TS_H_ERR)] = err;
      img[ts_hdr(TS_H_QSEQ)] = qseq, img[ts_hdr(TS_H_MB)] = mb, img[ts_hdr(TS_H_MT)] = mt;
      img[ts_hdr(TS_H_NBUF)] = nbuf, img[ts_hdr(TS_H_BHI)] = bhi;
    }
#pragma unroll
    for (uint32_t i = 0; i < R; ++i) {
      img[ts_reg(TS_P_KEY, i, lid)] = pk[i], img[ts_reg(TS_P_CLOCK, i, lid)] = pc[i];
      img[ts_reg(TS_P_DOT, i, lid)] = pd[i], img[ts_reg(TS_P_ARRIVAL, i, lid)] = pa[i];
      if constexpr (MULTI) {
        img[ts_reg(TS_P_META, i, lid)] = pm[i];
        img[ts_reg(TS_P_RING_KEY, i, lid)] = sk[i], img[ts_reg(TS_P_RING_DOT, i, lid)] = sd[i];
      }
      if constexpr (SHARDS) img[ts_reg(TS_P_SHARDS, i, lid)] = pz[i];
    }
    if constexpr (MULTI && !SHARDS) img[ts_buf(0, lid)] = bk, img[ts_buf(1, lid)] = bd, img[ts_buf(2, lid)] = bc;
  }
}

}  // namespace table
}  // namespace fx

using namespace fx;

extern "C" size_t fx_table_state_bytes(uint32_t n, uint32_t keys, uint32_t lanes) {
  (void)n;  // the table keeps 16 voter columns whatever n
  return table::hbm_words(keys) * 4 * lanes;
}

extern "C" size_t fx_table_state_bytes_ps(uint32_t n, uint32_t keys, uint32_t lanes) {
  (void)n;  // the votes tables and FX_TABLE_PS_HBM_BUFFERED (key, dot, count) entries
  return (table::hbm_words(keys) + 3u * FX_TABLE_PS_HBM_BUFFERED) * 4 * lanes;
}

// fx_table_execute (nkeys NULL, the single-key kernels), fx_table_execute_mk
// and fx_table_execute_ps (shards: the nkeys plane holds FX_TABLE_PS_WORD)
static int table_execute(const fx_table_batch* in, const uint32_t* nkeys, bool multi, const fx_order_batch* out,
                         uint32_t* stable_clock, const uint32_t* stream_map, uint32_t num_lanes, uint32_t tier,
                         void* state, uint32_t flags, void* hip_stream, bool shards = false,
                         uint32_t* stable_sent = nullptr) {
  if (multi && !nkeys) return FX_ERR_INVALID_ARG;
  if (!in || !out || !in->hdr || !in->dot || !in->clock || !in->votes || !out->order || !out->release ||
      !out->nexec || !out->err)
    return FX_ERR_INVALID_ARG;
  if (in->n < 1 || in->n > table::NV || in->stability_threshold < 1 || in->stability_threshold > in->n ||
      in->vmax < 1 || in->vmax > FX_TABLE_MAX_VOTES || in->keys < 1 || in->keys > FX_TABLE_MAX_KEYS ||
      in->steps >= (1u << 26) || (flags & ~FX_FLAG_EXECUTE_AT_COMMIT))
    return FX_ERR_INVALID_ARG;
  if (!stream_map && num_lanes > in->num_streams) return FX_ERR_INVALID_ARG;
  if (tier > FX_TABLE_TIER_HBM || (tier == FX_TABLE_TIER_HBM) != (state != nullptr)) return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (tier == FX_TABLE_TIER_ONCHIP && in->keys > FX_TABLE_ONCHIP_KEYS) return FX_ERR_UNSUPPORTED;
  if (num_lanes == 0) return FX_OK;
  table::TArgs a{};
  a.hdr = in->hdr;
  a.dot = in->dot;
  a.clock = in->clock;
  a.votes = in->votes;
  a.lengths = in->lengths;
  a.S = in->num_streams;
  a.steps = in->steps;
  a.n = in->n;
  a.keys = in->keys;
  a.vmax = in->vmax;
  a.thr = in->stability_threshold;
  a.plane = fx_plane_words(in->num_streams, in->steps);
  a.order = out->order;
  a.release = out->release;
  a.nexec = out->nexec;
  a.err = out->err;
  a.stable = stable_clock;
  a.stream_map = stream_map;
  a.num_lanes = num_lanes;
  a.state = (uint32_t*)state;
  a.flags = flags;
  a.nkeys = nkeys;
  a.sent = stable_sent;
  hipStream_t hs = (hipStream_t)hip_stream;
  fx::profile_slot_record(FX_PROFILE_SLOT_TABLE + tier, false, hs);
  constexpr uint32_t W = table::ONCHIP_WPB;
  const dim3 grid(xcd_grid(tier == FX_TABLE_TIER_HBM ? num_lanes : (num_lanes + W - 1u) / W));
  const size_t lds = (size_t)W * in->keys * 32u * 4u;
  if (tier == FX_TABLE_TIER_HBM) {
    if (shards) hipLaunchKernelGGL((table::k_table<true, table::HBM_R, 1, true, true>), grid, dim3(64), 0, hs, a);
    else if (multi) hipLaunchKernelGGL((table::k_table<true, table::HBM_R, 1, true>), grid, dim3(64), 0, hs, a);
    else hipLaunchKernelGGL((table::k_table<true, table::HBM_R, 1, false>), grid, dim3(64), 0, hs, a);
  } else {
    if (shards) hipLaunchKernelGGL((table::k_table<false, 1, W, true, true>), grid, dim3(64 * W), lds, hs, a);
    else if (multi) hipLaunchKernelGGL((table::k_table<false, 1, W, true>), grid, dim3(64 * W), lds, hs, a);
    else hipLaunchKernelGGL((table::k_table<false, 1, W, false>), grid, dim3(64 * W), lds, hs, a);
  }
  if (hipGetLastError() != hipSuccess) return FX_ERR_HIP;
  fx::profile_slot_record(FX_PROFILE_SLOT_TABLE + tier, true, hs);
  return FX_OK;
}

extern "C" int fx_table_execute(const fx_table_batch* in, const fx_order_batch* out, uint32_t* stable_clock,
                                const uint32_t* stream_map, uint32_t num_lanes, uint32_t tier, void* state,
                                uint32_t flags, void* hip_stream) {
  return table_execute(in, nullptr, false, out, stable_clock, stream_map, num_lanes, tier, state, flags, hip_stream);
}

extern "C" int fx_table_execute_mk(const fx_table_batch_mk* in, const fx_order_batch* out, uint32_t* stable_clock,
                                   const uint32_t* stream_map, uint32_t num_lanes, uint32_t tier, void* state,
                                   uint32_t flags, void* hip_stream) {
  if (!in) return FX_ERR_INVALID_ARG;
  return table_execute(&in->base, in->nkeys, true, out, stable_clock, stream_map, num_lanes, tier, state, flags,
                       hip_stream);
}

extern "C" int fx_table_execute_ps(const fx_table_batch_mk* in, const fx_order_batch* out, uint32_t* stable_clock,
                                   uint32_t* stable_sent, const uint32_t* stream_map, uint32_t num_lanes,
                                   uint32_t tier, void* state, uint32_t flags, void* hip_stream) {
  if (!in) return FX_ERR_INVALID_ARG;
  return table_execute(&in->base, in->nkeys, true, out, stable_clock, stream_map, num_lanes, tier, state, flags,
                       hip_stream, true, stable_sent);
}

extern "C" size_t fx_table_session_bytes(uint32_t kind, uint32_t n, uint32_t keys, uint32_t num_streams) {
  (void)n;
  return kind > FX_TABLE_KIND_PS ? 0 : table::ts_stride(kind, keys) * 4 * num_streams;
}

// Rows [done, lengths[s]) of every stream from the state the call before left
// (table_state.h): the RESUME kernels, HBM tables only
extern "C" int fx_table_advance(const fx_table_batch_mk* in, uint32_t kind, const fx_order_batch* out,
                                uint32_t* stable_clock, uint32_t* stable_sent, void* state, uint32_t flags,
                                void* hip_stream) {
  if (!in || !out || kind > FX_TABLE_KIND_PS || !state || (flags & ~(FX_FLAG_INIT | FX_FLAG_EXECUTE_AT_COMMIT)))
    return FX_ERR_INVALID_ARG;
  const fx_table_batch& b = in->base;
  if (!b.hdr || !b.dot || !b.clock || !b.votes || !out->order || !out->release || !out->nexec || !out->err ||
      (kind != FX_TABLE_KIND_SINGLE && !in->nkeys) || (kind != FX_TABLE_KIND_PS && stable_sent))
    return FX_ERR_INVALID_ARG;
  if (b.n < 1 || b.n > table::NV || b.stability_threshold < 1 || b.stability_threshold > b.n || b.vmax < 1 ||
      b.vmax > FX_TABLE_MAX_VOTES || b.keys < 1 || b.keys > FX_TABLE_MAX_KEYS || b.steps >= (1u << 26))
    return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (b.num_streams == 0) return FX_OK;
  table::TArgs a{};
  a.hdr = b.hdr;
  a.dot = b.dot;
  a.clock = b.clock;
  a.votes = b.votes;
  a.lengths = b.lengths;
  a.S = b.num_streams;
  a.steps = b.steps;
  a.n = b.n;
  a.keys = b.keys;
  a.vmax = b.vmax;
  a.thr = b.stability_threshold;
  a.plane = fx_plane_words(b.num_streams, b.steps);
  a.order = out->order;
  a.release = out->release;
  a.nexec = out->nexec;
  a.err = out->err;
  a.stable = stable_clock;
  a.num_lanes = b.num_streams;
  a.state = (uint32_t*)state;
  a.flags = flags;
  a.nkeys = in->nkeys;
  a.sent = stable_sent;
  hipStream_t hs = (hipStream_t)hip_stream;
  constexpr uint32_t SLOT = FX_PROFILE_SLOT_TABLE + 2u;
  fx::profile_slot_record(SLOT, false, hs);
  const dim3 grid(xcd_grid(b.num_streams));
  if (kind == FX_TABLE_KIND_PS)
    hipLaunchKernelGGL((table::k_table<true, table::HBM_R, 1, true, true, true>), grid, dim3(64), 0, hs, a);
  else if (kind == FX_TABLE_KIND_MK)
    hipLaunchKernelGGL((table::k_table<true, table::HBM_R, 1, true, false, true>), grid, dim3(64), 0, hs, a);
  else
    hipLaunchKernelGGL((table::k_table<true, table::HBM_R, 1, false, false, true>), grid, dim3(64), 0, hs, a);
  if (hipGetLastError() != hipSuccess) return FX_ERR_HIP;
  fx::profile_slot_record(SLOT, true, hs);
  return FX_OK;
}

// Every stream at ONCHIP (when the keys fit), then the ones that ran out of
// capacity at HBM.  Synchronous.
static int table_run(const fx_table_batch* in, const uint32_t* nkeys, bool multi, const fx_order_batch* out,
                     uint32_t* stable_clock, uint32_t flags, void* hip_stream, uint32_t* reruns, bool shards = false,
                     uint32_t* stable_sent = nullptr) {
  if (reruns) *reruns = 0;
  if (!in || !out) return FX_ERR_INVALID_ARG;
  // the arguments and the device, checked by an empty launch (a key count
  // beyond the ONCHIP tier's only skips that tier)
  const int st0 =
      table_execute(in, nkeys, multi, out, stable_clock, nullptr, 0, FX_TABLE_TIER_ONCHIP, nullptr, flags, hip_stream,
                    shards, stable_sent);
  if (st0 && st0 != FX_ERR_UNSUPPORTED) return st0;
  const uint32_t S = in->num_streams;
  hipStream_t hs = (hipStream_t)hip_stream;
  std::vector<uint32_t> err(S), todo;
  bool first = true;
  uint32_t rr = 0;
  for (uint32_t tier = FX_TABLE_TIER_ONCHIP; tier <= FX_TABLE_TIER_HBM; ++tier) {
    if (tier == FX_TABLE_TIER_ONCHIP && in->keys > FX_TABLE_ONCHIP_KEYS) continue;
    if (!first && todo.empty()) break;
    const uint32_t L = first ? S : (uint32_t)todo.size();
    std::lock_guard<std::recursive_mutex> lock(scratch_mutex());
    uint32_t* dmap = nullptr;
    void* dstate = nullptr;
    if (!first) {
      dmap = (uint32_t*)scratch(SCRATCH_TIERED_MAP, (size_t)L * 4);
      if (!dmap) return FX_ERR_HIP;
      if (hipMemcpyAsync(dmap, todo.data(), (size_t)L * 4, hipMemcpyHostToDevice, hs) != hipSuccess) return FX_ERR_HIP;
      rr += L;
    }
    if (tier == FX_TABLE_TIER_HBM) {
      dstate = scratch(SCRATCH_TIERED_STATE, shards ? fx_table_state_bytes_ps(in->n, in->keys, L)
                                                    : fx_table_state_bytes(in->n, in->keys, L));
      if (!dstate) return FX_ERR_HIP;
    }
    const int st = table_execute(in, nkeys, multi, out, stable_clock, dmap, L, tier, dstate, flags, hip_stream, shards,
                                 stable_sent);
    if (st) return st;
    if (S && (hipMemcpyAsync(err.data(), out->err, (size_t)S * 4, hipMemcpyDeviceToHost, hs) != hipSuccess ||
              hipStreamSynchronize(hs) != hipSuccess))
      return FX_ERR_HIP;
    first = false;
    todo.clear();
    for (uint32_t s = 0; s < S; ++s)
      if (err[s] == FX_ERR_CAPACITY) todo.push_back(s);
  }
  if (reruns) *reruns = rr;
  for (uint32_t s = 0; s < S; ++s)
    if (err[s]) return (int)err[s];
  return FX_OK;
}

extern "C" int fx_table_run(const fx_table_batch* in, const fx_order_batch* out, uint32_t* stable_clock,
                            uint32_t flags, void* hip_stream, uint32_t* reruns) {
  return table_run(in, nullptr, false, out, stable_clock, flags, hip_stream, reruns);
}

extern "C" int fx_table_run_mk(const fx_table_batch_mk* in, const fx_order_batch* out, uint32_t* stable_clock,
                               uint32_t flags, void* hip_stream, uint32_t* reruns) {
  if (reruns) *reruns = 0;
  if (!in) return FX_ERR_INVALID_ARG;
  return table_run(&in->base, in->nkeys, true, out, stable_clock, flags, hip_stream, reruns);
}

extern "C" int fx_table_run_ps(const fx_table_batch_mk* in, const fx_order_batch* out, uint32_t* stable_clock,
                               uint32_t* stable_sent, uint32_t flags, void* hip_stream, uint32_t* reruns) {
  if (reruns) *reruns = 0;
  if (!in) return FX_ERR_INVALID_ARG;
  return table_run(&in->base, in->nkeys, true, out, stable_clock, flags, hip_stream, reruns, true, stable_sent);
}
