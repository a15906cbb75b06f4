// table_group_synth.hip — closed-loop shard groups generated on the device
// (fx_table_group_synth_count / fx_table_group_synth_generate; the model:
// fx_table_group_synth.h).
//
// A command's commit clock is the highest proposal over all its shards, so a
// group is sequential as a whole: one lane per group, one wavefront per 64
// groups.  Two launches of the same walk, as table_synth.hip:
// k_table_group_synth<.., false> counts per (shard, delivery slot) the events
// and the words of the target lists into scratch[shard][slot][group]
// (slot-major: a wavefront's lanes touch adjacent words), turns the event
// counts into first rows and leaves per stream the length and the rows it can
// be handled in, per group the words of its lists.  The host, at the
// synchronisation the counting pass has anyway, makes the exclusive prefix of
// those over the groups: every group's base in targets.
// k_table_group_synth<.., true> turns the list counts into cursors from that
// base, walks the same draws and stores.  Per-group state
// (clocks[shard][key][process], the coordinators' command counts) is word w of
// lane l at LDS word 64 w + l while shards * keys * n + n <=
// FX_TABLE_SYNTH_ONCHIP_WORDS, else at scratch[w][group].  No lane reads
// another lane's words: no barrier, no cross-lane operation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "fx_table_group_synth.h"

namespace {

struct GroupSynthArgs {
  fx_table_group_synth_params p;
  uint32_t* rows;     // [shards * nslots][gpad]
  uint32_t* lists;    // [shards * nslots][gpad]
  uint32_t* handled;  // [shards][gpad]: rows of the messages, then rows the stream is handled in
  uint32_t* total;    // [gpad] words of the group's lists
  uint32_t* base;     // [gpad] the group's first word in targets
  uint32_t* lens;     // [shards * gpad] the lengths of a generate call until it is known to fit
  uint32_t* state;    // [tg_state_words][gpad], off-chip state only
  uint32_t* lengths;  // [groups * shards]
  uint32_t gpad;
  fx::TgOut out;      // EMIT only (ev.stream filled in per lane)
};

template <bool LDS, bool EMIT>
__global__ __launch_bounds__(64) void k_table_group_synth(const GroupSynthArgs a) {
  extern __shared__ uint32_t lds_state[];
  const uint32_t g = blockIdx.x * 64u + threadIdx.x;
  if (g >= a.p.groups) return;  // pad lanes: nothing of theirs exists
  const fx::TgGroup tg = fx::tg_group(a.p, g);
  const uint32_t P = tg.P, per = P * tg.nslots;
  const fx::TsWords rows{a.rows + g, a.gpad}, lists{a.lists + g, a.gpad}, handled{a.handled + g, a.gpad};
  const fx::TsWords state = LDS ? fx::TsWords{lds_state + threadIdx.x, 64} : fx::TsWords{a.state + g, a.gpad};
  fx::TgOut out = a.out;
  out.ev.stream = g * P;
  if (EMIT) fx::tg_prefix_lists(lists, per, a.base[g]);
  fx::tg_walk<EMIT>(tg, state, rows, lists, handled, out);
  if (!EMIT) {
    for (uint32_t h = 0; h < P; ++h) {
      const uint32_t len = fx::ts_prefix(rows.from((size_t)h * tg.nslots), tg.nslots);
      a.lengths[g * P + h] = len;
      handled[h] = handled[h] + len;
    }
    a.total[g] = fx::tg_list_words(lists, per);
  }
}

// the state on chip while it fits, else in scratch
template <bool EMIT>
bool launch(const GroupSynthArgs& a, hipStream_t hs) {
  const uint32_t words = fx::tg_state_words(a.p);
  const dim3 grid(a.gpad / 64u);
  if (words <= FX_TABLE_SYNTH_ONCHIP_WORDS)
    hipLaunchKernelGGL((k_table_group_synth<true, EMIT>), grid, dim3(64), (size_t)words * 256u, hs, a);
  else
    hipLaunchKernelGGL((k_table_group_synth<false, EMIT>), grid, dim3(64), 0, hs, a);
  return hipGetLastError() == hipSuccess;
}

// Both passes share the arguments; the counting pass is waited for.
int count_pass(const fx_table_group_synth_params* p, uint32_t* lengths_dev, void* scratch, hipStream_t hs,
               GroupSynthArgs& a, uint32_t* max_len, uint32_t* steps_out, uint64_t* targets_words) {
  a.p = *p;
  const uint32_t Gn = p->groups, P = p->shards;
  const size_t gpad = ((size_t)Gn + 63u) / 64u * 64u, per = (size_t)P * fx::ts_slots(*p);
  a.gpad = (uint32_t)gpad;
  a.rows = (uint32_t*)scratch;
  a.lists = a.rows + per * gpad;
  a.handled = a.lists + per * gpad;
  a.total = a.handled + (size_t)P * gpad;
  a.base = a.total + gpad;
  a.lens = a.base + gpad;
  a.state = a.lens + (size_t)P * gpad;
  a.lengths = lengths_dev;
  a.out = fx::TgOut{};
  if (max_len) *max_len = 0;
  if (steps_out) *steps_out = 1;
  if (targets_words) *targets_words = 0;
  if (Gn == 0) return FX_OK;
  if (hipMemsetAsync(a.rows, 0, (2u * per + P + 2u) * gpad * 4, hs) != hipSuccess) return FX_ERR_HIP;
  if (!launch<false>(a, hs)) return FX_ERR_HIP;
  const size_t S = (size_t)Gn * P;
  std::vector<uint32_t> len(S), counts(((size_t)P + 1u) * gpad), base(Gn);
  if (hipMemcpyAsync(len.data(), lengths_dev, S * 4, hipMemcpyDeviceToHost, hs) != hipSuccess ||
      hipMemcpyAsync(counts.data(), a.handled, counts.size() * 4, hipMemcpyDeviceToHost, hs) != hipSuccess ||
      hipStreamSynchronize(hs) != hipSuccess)
    return FX_ERR_HIP;
  uint32_t rows_out = 1;
  for (uint32_t h = 0; h < P; ++h)
    rows_out = std::max(rows_out, *std::max_element(counts.begin() + h * gpad, counts.begin() + h * gpad + Gn));
  uint64_t run = 0;
  for (uint32_t g = 0; g < Gn; ++g) {
    base[g] = (uint32_t)run;
    run += counts[(size_t)P * gpad + g];
  }
  if (max_len) *max_len = *std::max_element(len.begin(), len.end());
  if (steps_out) *steps_out = rows_out;
  if (targets_words) *targets_words = run;
  // every group's base in targets (beyond 32 bits no caller's targets can hold the lists)
  if (run <= 0xFFFFFFFFull && (hipMemcpyAsync(a.base, base.data(), (size_t)Gn * 4, hipMemcpyHostToDevice, hs) != hipSuccess ||
                               hipStreamSynchronize(hs) != hipSuccess))
    return FX_ERR_HIP;
  return FX_OK;
}

}  // namespace

extern "C" int fx_table_group_synth_count(const fx_table_group_synth_params* p, uint32_t* lengths_dev, void* scratch,
                                          void* hip_stream, uint32_t* max_len, uint32_t* steps_out,
                                          uint64_t* targets_words) {
  const int st = fx::tg_check(p);
  if (st) return st;
  if (!lengths_dev || !scratch) return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  GroupSynthArgs a;
  return count_pass(p, lengths_dev, scratch, (hipStream_t)hip_stream, a, max_len, steps_out, targets_words);
}

extern "C" int fx_table_group_synth_generate(const fx_table_group_synth_params* p,
                                             const fx_table_group_synth_planes* o, uint32_t steps,
                                             uint32_t targets_words, void* scratch, void* hip_stream) {
  int st = fx::tg_check(p);
  if (st) return st;
  if (!o || !o->hdr || !o->dot || !o->clock || !o->votes || !o->nkeys || !o->route || !o->lengths ||
      (!o->targets && targets_words) || !scratch)
    return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  hipStream_t hs = (hipStream_t)hip_stream;
  GroupSynthArgs a;
  uint32_t longest = 0;
  uint64_t lists = 0;
  // the lengths stay in scratch until the call is known to fit
  const size_t gpad = ((size_t)p->groups + 63u) / 64u * 64u;
  uint32_t* lens = (uint32_t*)scratch + (2u * (size_t)p->shards * fx::ts_slots(*p) + p->shards + 2u) * gpad;
  st = count_pass(p, lens, scratch, hs, a, &longest, nullptr, &lists);
  if (st) return st;
  if (longest > steps || lists > targets_words) return FX_ERR_CAPACITY;  // (nothing of the caller's is written)
  if (p->groups && hipMemcpyAsync(o->lengths, lens, (size_t)p->groups * p->shards * 4, hipMemcpyDeviceToDevice, hs) !=
                       hipSuccess)
    return FX_ERR_HIP;
  // rows no stream reaches and the pad streams of the last tile: zero, no route
  const size_t plane = fx_plane_words(p->groups * p->shards, steps);
  if (plane == 0) return FX_OK;
  a.out = fx::TgOut{{o->hdr, o->dot, o->clock, o->votes, o->nkeys, plane, steps, 0}, o->route, o->targets, targets_words};
  const auto set = [hs](void* at, int byte, size_t bytes) { return hipMemsetAsync(at, byte, bytes, hs) == hipSuccess; };
  if (!fx::ts_clear_planes(set, a.out.ev, p->fast_quorum, o->route)) return FX_ERR_HIP;
  return launch<true>(a, hs) ? FX_OK : FX_ERR_HIP;
}
