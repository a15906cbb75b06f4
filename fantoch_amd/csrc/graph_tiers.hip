// graph_tiers.hip — the graph executor's tiers in one table, and what reads
// it here: fx_tier_query, fx_batch_state_bytes, fx_batch_execute and
// fx_batch_run_tiered (the drop-in handle reads it in executor_host.cpp).  The
// tiers themselves live one per file (graph_exec: the three slot tiers,
// graph_group, graph_wave, graph_lane, graph_split, graph_wide).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "fantoch_amd.h"
#include "fx_internal.h"

namespace fx {

// Faces that do not ask for n, as the table's members.
template <auto F> size_t by_lanes(uint32_t, uint32_t lanes) { return F(lanes); }
template <auto F>
uint32_t by_lane(const uint32_t* block, uint32_t, uint32_t lane, uint32_t* dots, uint32_t* waits, uint32_t cap) {
  return F(block, lane, dots, waits, cap);
}
template <uint32_t TIER>
constexpr TierDesc slot_tier(uint32_t next, uint32_t next_resumable, bool init_needs_state) {
  using S = SlotTier<TIER>;
  return {S::info, MAX_DEPS, next, next_resumable, init_needs_state, S::state_bytes, S::launch, S::decode_pending};
}

// Indexed by FX_TIER_*: info, max_deps, next, next_resumable, init_needs_state,
// state_bytes, launch, decode_pending.
//
// max_deps decides where a batch starts: fx_batch_run_tiered and the drop-in
// handle's flush() both move a batch whose widest Add the tier cannot read to
// FX_TIER_LDS_LARGE.  The handle asks at whatever tier it stands on, which is
// only ever GROUP, WAVE, LDS_LARGE, GLOBAL or WIDE_HBM; the last three read
// every Add a batch can hold (MAX_DEPS), so for them the rule never fires.
//
// Host data: left to itself the device pass would emit the array too (a const
// with a constant initialiser) and look for device copies of the host
// functions it names.
#if !defined(__HIP_DEVICE_COMPILE__)
const TierDesc TIERS[FX_NUM_TIERS] = {
    {[](uint32_t) { return fx_tier_info{GROUP_LANES, GROUP_SLOTS, GROUP_WINDOW_BITS, group_state_words_per_stream()}; },
     GROUP_LANES, FX_TIER_LDS_LARGE, FX_TIER_LDS_LARGE, false, by_lanes<group_state_bytes>, launch_group,
     by_lane<group_decode_pending>},  // FX_TIER_GROUP
    slot_tier<FX_TIER_LDS_LARGE>(FX_TIER_GLOBAL, FX_TIER_GLOBAL, false),
    // the HBM slots are the tier's working memory; the LDS wide tier cannot resume
    slot_tier<FX_TIER_GLOBAL>(FX_TIER_WIDE, FX_TIER_WIDE_HBM, true),
    slot_tier<FX_TIER_LANE>(FX_TIER_LDS_LARGE, FX_TIER_LDS_LARGE, false),
    {[](uint32_t) { return fx_tier_info{8, WAVE_SLOTS, WAVE_WINDOW_BITS, wave_state_words_per_stream()}; },
     WAVE_MAX_DEPS, FX_TIER_GLOBAL, FX_TIER_GLOBAL, false, by_lanes<wave_state_bytes>, launch_wave,
     by_lane<wave_decode_pending>},  // FX_TIER_WAVE
    // FX_TIER_LANE_REG: launch_lane also refuses planes beyond its 32-bit offsets, which the rule leaves to it
    {[](uint32_t) { return fx_tier_info{8, LANE_SLOTS, LANE_WINDOW_BITS, lane_state_words_per_stream()}; },
     LANE_MAX_DEPS, FX_TIER_LDS_LARGE, FX_TIER_LDS_LARGE, false, by_lanes<lane_state_bytes>, launch_lane,
     by_lane<lane_decode_pending>},
    // FX_TIER_SPLIT: the smaller of its two tiers' limits; `state` is scheduling scratch, not resumable state
    {[](uint32_t) {
       return fx_tier_info{8, std::min(LANE_SLOTS, GROUP_SLOTS), std::min(LANE_WINDOW_BITS, GROUP_WINDOW_BITS), 0};
     },
     GROUP_LANES, FX_TIER_LDS_LARGE, FX_TIER_LDS_LARGE, true, by_lanes<split_scratch_bytes>, launch_split, nullptr},
    // FX_TIER_WIDE: tables in LDS, nothing saved
    {[](uint32_t) { return fx_tier_info{8, 512, 1024, 0}; },
     MAX_DEPS, FX_TIER_WIDE_HBM, FX_TIER_WIDE_HBM, false, [](uint32_t, uint32_t) { return (size_t)0; },
     [](const KArgs& a, hipStream_t s) { return launch_wide(a, false, s); }, nullptr},
    // FX_TIER_WIDE_HBM: the working tables, one block per stream
    {[](uint32_t n) { return fx_tier_info{8, 16384, 32768, (uint32_t)(wide_hbm_state_bytes(n, 1) / 4)}; },
     MAX_DEPS, FX_NUM_TIERS, FX_NUM_TIERS, true, wide_hbm_state_bytes,
     [](const KArgs& a, hipStream_t s) { return launch_wide(a, true, s); },
     [](const uint32_t* block, uint32_t n, uint32_t, uint32_t* dots, uint32_t* waits, uint32_t cap) {
       return wide_decode_pending(block, n, dots, waits, cap);
     }},
};
#endif

}  // namespace fx

using namespace fx;

extern "C" {

int fx_tier_query(uint32_t tier, uint32_t n, fx_tier_info* out) {
  if (!out || tier >= FX_NUM_TIERS) return FX_ERR_INVALID_ARG;
  *out = TIERS[tier].info(n);
  return n >= 1 && n <= out->max_sources ? FX_OK : FX_ERR_INVALID_ARG;
}

size_t fx_batch_state_bytes(uint32_t tier, uint32_t n, uint32_t lanes) {
  return tier < FX_NUM_TIERS ? TIERS[tier].state_bytes(n, lanes) : 0;
}

static int check_batch(const fx_stream_batch* in, const fx_order_batch* out) {
  if (!in || !out || !in->dot || !in->hdr || (in->dmax && !in->deps) || !out->order ||
      !out->release || !out->nexec || !out->err)
    return FX_ERR_INVALID_ARG;
  if (in->n < 1 || in->n > 8 || in->steps >= (1u << 26) || in->dmax > MAX_DEPS) return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  return FX_OK;
}

int fx_batch_execute(const fx_stream_batch* in, const fx_order_batch* out, uint32_t tier,
                     const uint32_t* stream_map, uint32_t num_lanes, void* state,
                     uint32_t step_begin, uint32_t step_end, uint32_t flags,
                     const uint32_t* init_frontier, void* hip_stream) {
  int st = check_batch(in, out);
  if (st) return st;
  if (step_end > in->steps || step_begin > step_end) return FX_ERR_INVALID_ARG;
  if (!(flags & FX_FLAG_INIT) && !state) return FX_ERR_INVALID_ARG;
  if ((flags & FX_FLAG_SAVE_STATE) && !state) return FX_ERR_INVALID_ARG;
  if (!stream_map && num_lanes > in->num_streams) return FX_ERR_INVALID_ARG;
  // the split tier schedules whole batches: no map, no resumable state
  if (tier == FX_TIER_SPLIT &&
      (stream_map || num_lanes != in->num_streams || !state || !(flags & FX_FLAG_INIT) ||
       (flags & FX_FLAG_SAVE_STATE)))
    return FX_ERR_INVALID_ARG;
  KArgs a = kargs_of(*in, *out);
  a.stream_map = stream_map;
  a.num_lanes = num_lanes;
  a.state = (uint32_t*)state;
  a.step_begin = step_begin;
  a.step_end = step_end;
  a.flags = flags;
  a.init_frontier = init_frontier;
  if (flags & FX_FLAG_PARTIAL) return FX_ERR_INVALID_ARG;  // fx_batch_execute_partial
  hipStream_t hs = (hipStream_t)hip_stream;
  if ((st = profile_exec_begin(hs))) return st;
  profile_slot_record(tier, false, hs);
  if (tier >= FX_NUM_TIERS) return FX_ERR_INVALID_ARG;
  st = TIERS[tier].launch(a, hs);
  profile_exec_end(st == FX_OK, hs);
  if (st == FX_OK) profile_slot_record(tier, true, hs);
  return st;
}

size_t fx_partial_state_bytes(uint32_t n, uint32_t num_streams) { return wide_partial_state_bytes(n, num_streams); }

int fx_batch_execute_partial(const fx_stream_batch* in, const fx_order_batch* out, void* state,
                             uint32_t step_begin, uint32_t step_end, uint32_t flags,
                             const uint32_t* init_frontier, uint32_t* req, uint32_t req_cap, void* hip_stream) {
  int st = check_batch(in, out);
  if (st) return st;
  if (step_end > in->steps || step_begin > step_end || !state || !req || req_cap == 0) return FX_ERR_INVALID_ARG;
  if (flags & ~(FX_FLAG_INIT | FX_FLAG_SAVE_STATE)) return FX_ERR_INVALID_ARG;
  KArgs a = kargs_of(*in, *out);
  a.state = (uint32_t*)state;
  a.step_begin = step_begin;
  a.step_end = step_end;
  a.flags = flags | FX_FLAG_PARTIAL;
  a.init_frontier = init_frontier;
  a.req = req;
  a.req_cap = req_cap;
  return launch_wide(a, true, (hipStream_t)hip_stream);
}

}  // extern "C"

namespace fx {

// fx_batch_run_tiered: the first tier for all (or for the streams in `only`),
// then run_ladder's reruns up the escalation chain.
int run_tiered(const fx_stream_batch* in, const fx_order_batch* out, uint32_t flags, void* hip_stream,
               const std::vector<uint32_t>* only, uint32_t* tier_counts) {
  int st = check_batch(in, out);
  if (st) return st;
  flags |= FX_FLAG_INIT;
  flags &= ~FX_FLAG_SAVE_STATE;
  const uint32_t ft = (flags >> FX_FLAG_TIER_SHIFT) & 15u;
  flags &= ~(15u << FX_FLAG_TIER_SHIFT);
  uint32_t first = ft ? ft - 1u : (uint32_t)FX_TIER_DEFAULT;
  if (first >= FX_NUM_TIERS) return FX_ERR_INVALID_ARG;
  if (only && first == FX_TIER_SPLIT) first = FX_TIER_GROUP;  // the split tier takes whole batches
  // a tier that cannot read the widest Add gives way to the narrowest that reads any
  if (in->dmax > TIERS[first].max_deps) first = FX_TIER_LDS_LARGE;
  if (tier_counts)
    for (uint32_t t = 0; t < FX_NUM_TIERS; ++t) tier_counts[t] = 0;
  std::vector<uint32_t> chain;
  for (uint32_t tier = first; tier < FX_NUM_TIERS; tier = TIERS[tier].next)
    if (tier != FX_TIER_WIDE || wide_lds_fits(in->n, in->dmax)) chain.push_back(tier);  // else straight to the HBM tables
  const LadderRun r = run_ladder(
      in->num_streams, only, out->err, (hipStream_t)hip_stream, chain, true,
      [&](uint32_t tier, uint32_t L) {
        return TIERS[tier].init_needs_state ? fx_batch_state_bytes(tier, in->n, L) : (size_t)0;
      },
      [&](uint32_t tier, const uint32_t* map, uint32_t L, void* state) {
        return fx_batch_execute(in, out, tier, map, L, state, 0, in->steps, flags, nullptr, hip_stream);
      });
  if (tier_counts)
    for (size_t i = 0; i < chain.size(); ++i) tier_counts[chain[i]] = r.lanes[i];
  return r.status ? r.status : r.lowest;
}

}  // namespace fx

extern "C" int fx_batch_run_tiered(const fx_stream_batch* in, const fx_order_batch* out, uint32_t flags,
                                   void* hip_stream, uint32_t* tier_counts) {
  return fx::run_tiered(in, out, flags, hip_stream, nullptr, tier_counts);
}
