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
#include "fx_wave.h"
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

// GROUP (fx_table_run_groups): what the group kernel has beside TArgs.  The
// input planes have a.steps rows, every output plane steps_out rows.
struct GArgs {
  const uint32_t* route;
  const uint32_t* targets;
  uint32_t shards, groups, steps_out, max_rounds;
  uint32_t* hsrc;
  uint32_t* hdot;
  uint32_t* hlen;
  uint32_t* rounds;
};
// LDS of the group kernel, per shard executor: the inbox -- GI entries of (due
// round, send index, key, dot), field c of entry e at [c * GI + e], free while
// its due round is NONE -- that only its own wavefront touches, and the sends
// of the round -- GS entries of (step, handled row, route, dot), field c of
// entry e at [c * GS + e] -- that every
// wavefront of the group reads after the round's barrier; then one word per
// shard for the number of sends and one for "has events left"
constexpr uint32_t GI = FX_TABLE_GROUP_INBOX, GS = FX_TABLE_GROUP_SENDS;
constexpr uint32_t G_SHARD_WORDS = 4u * GI + 4u * GS + 2u;
static_assert(GI % 64u == 0 && GS == 64u, "an inbox row and the send list are one entry per lane");
constexpr uint32_t TGT_KEY = 0x00FFFFFFu;
__host__ __device__ constexpr inline uint32_t tgt_shard(uint32_t w) { return (w >> 24) & 7u; }
__host__ __device__ constexpr inline uint32_t tgt_delay(uint32_t w) { return w >> 27; }

// HBM table of one stream: row j, column v at [j * NV + v]; rows 0..keys-1
// the frontiers, row keys + k * WB + i word i of key k's windows
__host__ __device__ constexpr inline size_t hbm_words(uint32_t keys) { return (size_t)keys * NV * (1u + WB); }
static_assert(TS_NV == NV && TS_WB == WB && ts_votes_words(999) == hbm_words(999), "table_state.h describes these tables");

// MULTI: an op's meta word = seq (26 bits: steps < 2^26) | state << 26 | (nkeys - 1) << 28
constexpr uint32_t SEQ_MASK = (1u << 26) - 1u;
constexpr uint32_t ST_TABLE = 0, ST_QUEUED = 1, ST_TRIED = 2, ST_TOLD = 3;
__device__ __forceinline__ uint32_t m_state(uint32_t m) { return (m >> 26) & 3u; }
__device__ __forceinline__ uint32_t m_nkeys(uint32_t m) { return (m >> 28) + 1u; }
__device__ __forceinline__ uint32_t m_with(uint32_t m, uint32_t state) { return (m & ~(3u << 26)) | (state << 26); }

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
//
// GROUP (fx_table_run_groups, k_table_group): the wavefronts of a workgroup are the shard
// executors of one group and the event loop is the closed loop of DESIGN.md
// C14, a round per iteration, see below.
template <bool HBM, uint32_t R, uint32_t WPB, bool MULTI, bool SHARDS = false, bool RESUME = false>
__global__ __launch_bounds__(64 * WPB) void k_table(TArgs a) {
  constexpr bool GROUP = false;
  const GArgs ga{};
#include "table_wave.inc"
}

// fx_table_run_groups: one workgroup per group, one wavefront per shard executor
__global__ __launch_bounds__(64 * FX_TABLE_MAX_CMD_SHARDS) void k_table_group(TArgs a, GArgs ga) {
  constexpr bool GROUP = true, HBM = true, MULTI = true, SHARDS = true, RESUME = false;
  constexpr uint32_t R = HBM_R, WPB = 1;
#include "table_wave.inc"
}

// The input check of fx_table_run_groups, one lane per own row: a bad row
// stops its stream before round 0, so k_table_group may trust the routes
__global__ __launch_bounds__(256) void k_table_group_check(TArgs a, GArgs ga, uint32_t targets_words) {
  const size_t tid = (size_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t s = (uint32_t)(tid / a.steps), r = (uint32_t)(tid % a.steps);
  if (s >= a.S || r >= (a.lengths ? min(a.lengths[s], a.steps) : a.steps)) return;
  const size_t at = fx_index(r, s, a.steps);
  const uint32_t h = a.hdr[at], shard = s % ga.shards;
  bool bad = h >> 24 == FX_TABLE_HDR_STABLE(0) >> 24;
  const uint32_t SH = FX_TABLE_PS_WORD_SHARDS(a.nkeys[at]);
  if (!bad && FX_TABLE_HDR_KIND(h) == FX_TABLE_ATTACHED && SH > 1u && SH <= FX_TABLE_MAX_CMD_SHARDS) {
    const uint32_t rt = ga.route[at];
    const uint32_t m = rt < targets_words ? ga.targets[rt] : 0u;
    bad = rt >= targets_words || m >= targets_words - rt;  // (rt == FX_TABLE_ROUTE_NONE among them)
    uint32_t seen = 0;
    for (uint32_t i = 0; !bad && i < m; ++i) {
      const uint32_t w = ga.targets[rt + 1u + i];
      bad = tgt_shard(w) >= ga.shards || tgt_shard(w) == shard || (w & TGT_KEY) >= a.keys;
      seen |= 1u << tgt_shard(w);
    }
    bad = bad || (uint32_t)__builtin_popcount(seen) != SH - 1u;
  }
  if (bad) a.err[s] = FX_ERR_INVALID_ARG;
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

// The pointers and the shape every entry point asks of a batch and its outputs
static bool table_batch_ok(const fx_table_batch& b, const fx_order_batch& out) {
  return b.hdr && b.dot && b.clock && b.votes && out.order && out.release && out.nexec && out.err && b.n >= 1 &&
         b.n <= table::NV && b.stability_threshold >= 1 && b.stability_threshold <= b.n && b.vmax >= 1 &&
         b.vmax <= FX_TABLE_MAX_VOTES && b.keys >= 1 && b.keys <= FX_TABLE_MAX_KEYS && b.steps < (1u << 26);
}

// The kernels' arguments: one lane per stream of the batch, no stream map
static table::TArgs table_args(const fx_table_batch& b, const uint32_t* nkeys, const fx_order_batch& out,
                               uint32_t* stable, uint32_t* sent, void* state, uint32_t flags) {
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
  a.order = out.order;
  a.release = out.release;
  a.nexec = out.nexec;
  a.err = out.err;
  a.stable = stable;
  a.num_lanes = b.num_streams;
  a.state = (uint32_t*)state;
  a.flags = flags;
  a.nkeys = nkeys;
  a.sent = sent;
  return a;
}

// fx_table_execute (nkeys NULL, the single-key kernels), fx_table_execute_mk
// and fx_table_execute_ps (shards: the nkeys plane holds FX_TABLE_PS_WORD)
static int table_execute(const fx_table_batch* in, const uint32_t* nkeys, bool multi, const fx_order_batch* out,
                         uint32_t* stable_clock, const uint32_t* stream_map, uint32_t num_lanes, uint32_t tier,
                         void* state, uint32_t flags, void* hip_stream, bool shards = false,
                         uint32_t* stable_sent = nullptr) {
  if (multi && !nkeys) return FX_ERR_INVALID_ARG;
  if (!in || !out || !table_batch_ok(*in, *out) || (flags & ~FX_FLAG_EXECUTE_AT_COMMIT)) return FX_ERR_INVALID_ARG;
  if (!stream_map && num_lanes > in->num_streams) return FX_ERR_INVALID_ARG;
  if (tier > FX_TABLE_TIER_HBM || (tier == FX_TABLE_TIER_HBM) != (state != nullptr)) return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (tier == FX_TABLE_TIER_ONCHIP && in->keys > FX_TABLE_ONCHIP_KEYS) return FX_ERR_UNSUPPORTED;
  if (num_lanes == 0) return FX_OK;
  table::TArgs a = table_args(*in, nkeys, *out, stable_clock, stable_sent, state, flags);
  a.stream_map = stream_map;
  a.num_lanes = num_lanes;
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
  if (!table_batch_ok(b, *out) || (kind != FX_TABLE_KIND_SINGLE && !in->nkeys) ||
      (kind != FX_TABLE_KIND_PS && stable_sent))
    return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (b.num_streams == 0) return FX_OK;
  const table::TArgs a = table_args(b, in->nkeys, *out, stable_clock, stable_sent, state, flags);
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

extern "C" size_t fx_table_groups_state_bytes(uint32_t n, uint32_t keys, uint32_t num_streams) {
  return fx_table_state_bytes_ps(n, keys, num_streams);
}

// The closed loop of every group in one launch (k_table_group), after the
// input check.  max_rounds 0: the cap that well-formed inputs cannot reach
extern "C" int fx_table_run_groups_capped(const fx_table_group_batch* in, const fx_table_group_out* out, void* state,
                                          uint32_t flags, void* hip_stream, uint32_t max_rounds) {
  if (!in || !out || !state || (flags & ~FX_FLAG_EXECUTE_AT_COMMIT)) return FX_ERR_INVALID_ARG;
  const fx_table_batch& b = in->own.base;
  if (!table_batch_ok(b, out->out) || !in->own.nkeys || !in->route || !in->targets || !out->stable_sent ||
      !out->handled_src || !out->handled_dot || !out->handled_len || !out->rounds || b.steps < 1)
    return FX_ERR_INVALID_ARG;
  if (in->shards < 1 || in->shards > FX_TABLE_MAX_CMD_SHARDS || b.num_streams % in->shards != 0 ||
      in->steps_out < 1 || in->steps_out >= (1u << 26))
    return FX_ERR_INVALID_ARG;
  const uint64_t rows = (uint64_t)b.num_streams * b.steps;  // the input check runs one lane per own row
  if ((rows + 255u) / 256u > 0x7FFFFFFFu) return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (b.num_streams == 0) return FX_OK;
  const table::TArgs a = table_args(b, in->own.nkeys, out->out, out->stable_clock, out->stable_sent, state, flags);
  table::GArgs ga{};
  ga.route = in->route;
  ga.targets = in->targets;
  ga.shards = in->shards;
  ga.groups = b.num_streams / in->shards;
  ga.steps_out = in->steps_out;
  // Rounds: while own events are left, at most `steps`; after that every round
  // has an undelivered message, a message is handled within 32 rounds of its
  // send plus the round of the send, and a shard handles at most steps_out
  // messages (then it stops with FX_ERR_ORDER_OVERFLOW)
  const uint64_t cap = (uint64_t)b.steps + 33ull * in->shards * in->steps_out + 1u;
  ga.max_rounds = max_rounds ? max_rounds : (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFFFu);
  ga.hsrc = out->handled_src;
  ga.hdot = out->handled_dot;
  ga.hlen = out->handled_len;
  ga.rounds = out->rounds;
  hipStream_t hs = (hipStream_t)hip_stream;
  constexpr uint32_t SLOT = FX_PROFILE_SLOT_TABLE + 3u;
  fx::profile_slot_record(SLOT, false, hs);
  if (hipMemsetAsync(a.err, 0, (size_t)b.num_streams * 4, hs) != hipSuccess) return FX_ERR_HIP;
  hipLaunchKernelGGL(table::k_table_group_check, dim3((uint32_t)((rows + 255u) / 256u)), dim3(256), 0, hs, a, ga,
                     in->targets_words);
  const size_t lds = (size_t)in->shards * table::G_SHARD_WORDS * 4u;
  hipLaunchKernelGGL(table::k_table_group, dim3(xcd_grid(ga.groups)), dim3(64u * in->shards), lds, hs, a, ga);
  if (hipGetLastError() != hipSuccess) return FX_ERR_HIP;
  fx::profile_slot_record(SLOT, true, hs);
  return FX_OK;
}

extern "C" int fx_table_run_groups(const fx_table_group_batch* in, const fx_table_group_out* out, void* state,
                                   uint32_t flags, void* hip_stream) {
  return fx_table_run_groups_capped(in, out, state, flags, hip_stream, 0);
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
  std::vector<uint32_t> chain;
  if (in->keys <= FX_TABLE_ONCHIP_KEYS) chain.push_back(FX_TABLE_TIER_ONCHIP);
  chain.push_back(FX_TABLE_TIER_HBM);
  const LadderRun r = run_ladder(
      in->num_streams, nullptr, out->err, (hipStream_t)hip_stream, chain, true,
      [&](uint32_t tier, uint32_t L) {
        if (tier != FX_TABLE_TIER_HBM) return (size_t)0;
        return shards ? fx_table_state_bytes_ps(in->n, in->keys, L) : fx_table_state_bytes(in->n, in->keys, L);
      },
      [&](uint32_t tier, const uint32_t* map, uint32_t L, void* state) {
        return table_execute(in, nkeys, multi, out, stable_clock, map, L, tier, state, flags, hip_stream, shards,
                             stable_sent);
      });
  if (r.status) return r.status;
  if (reruns) *reruns = r.reruns();
  return r.lowest;
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
