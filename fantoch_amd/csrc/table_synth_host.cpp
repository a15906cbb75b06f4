// table_synth_host.cpp — the host side of the synthetic Tempo vote streams
// (fx_table_synth.h): argument checks, the shape, and the host twin of the
// generator; below, the same for the closed-loop shard groups
// (fx_table_group_synth.h).  No HIP call in here, so the file also builds
// alone with a host compiler (tests/cpp/table_synth_host_check.cpp and
// tests/cpp/table_group_synth_host_check.cpp under the sanitizers).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the function attributes of fx_synth.h
#endif
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "fx_table_group_synth.h"
#include "fx_table_synth.h"

namespace {

// work(t, nt) on up to 16 threads: thread t of nt takes items t, t + nt, ...
// Every stream (group) writes its own words only.
template <class F>
void over_items(uint32_t items, F work) {
  const uint32_t nt = items < 64 ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (uint32_t t = 1; t < nt; ++t) th.emplace_back(work, t, nt);
  work(0u, nt);
  for (auto& x : th) x.join();
}

bool host_set(void* p, int byte, size_t bytes) {
  memset(p, byte, bytes);
  return true;
}

// The counting pass of every stream: lengths[s], and the longest.  slots_out
// (optional): the first rows of every stream's slots, [stream][slot].
void count_all(const fx_table_synth_params& p, uint32_t* lengths, uint32_t* max_len,
               std::vector<uint32_t>* slots_out) {
  const uint32_t S = p.streams, nslots = fx::ts_slots(p), words = fx::ts_state_words(p);
  if (slots_out) slots_out->assign((size_t)S * nslots, 0u);
  uint32_t longest[16] = {};  // per thread
  over_items(S, [&](uint32_t t, uint32_t nt) {
    std::vector<uint32_t> state(words), own(slots_out ? 0 : nslots);
    for (uint32_t s = t; s < S; s += nt) {
      uint32_t* sl = slots_out ? slots_out->data() + (size_t)s * nslots : own.data();
      if (!slots_out) std::fill(own.begin(), own.end(), 0u);
      const fx::TsWords slots{sl, 1};
      fx::ts_walk<false>(fx::ts_stream(p, s), fx::TsWords{state.data(), 1}, slots, fx::TsOut{});
      const uint32_t len = fx::ts_prefix(slots, nslots);
      if (lengths) lengths[s] = len;
      longest[t] = std::max(longest[t], len);
    }
  });
  if (max_len) *max_len = *std::max_element(longest, longest + 16);
}

}  // namespace

extern "C" {

int fx_table_synth_shape(const fx_table_synth_params* p, uint32_t* max_steps, uint32_t* vmax) {
  const int st = fx::ts_check(p);
  if (st) return st;
  if (max_steps) *max_steps = p->cmds * std::min(p->kmax, p->keys) * p->n;
  if (vmax) *vmax = p->fast_quorum;
  return FX_OK;
}

size_t fx_table_synth_scratch_bytes(const fx_table_synth_params* p) {
  if (fx::ts_check(p)) return 0;
  const size_t spad = ((size_t)p->streams + 63u) / 64u * 64u;
  const uint32_t words = fx::ts_state_words(*p);
  return 4u * spad * ((size_t)fx::ts_slots(*p) + (words > FX_TABLE_SYNTH_ONCHIP_WORDS ? words : 0u)) + 16u;
}

int fx_table_synth_lengths_host(const fx_table_synth_params* p, uint32_t* lengths, uint32_t* max_len) {
  const int st = fx::ts_check(p);
  if (st) return st;
  if (!lengths && p->streams) return FX_ERR_INVALID_ARG;
  count_all(*p, lengths, max_len, nullptr);
  return FX_OK;
}

int fx_table_synth_generate_host(const fx_table_synth_params* p, const fx_table_synth_planes* o, uint32_t steps) {
  const int st = fx::ts_check(p);
  if (st) return st;
  if (!o || !o->hdr || !o->dot || !o->clock || !o->votes || !o->lengths || (!o->nkeys && p->kmax > 1))
    return FX_ERR_INVALID_ARG;
  const uint32_t S = p->streams, nslots = fx::ts_slots(*p), words = fx::ts_state_words(*p);
  std::vector<uint32_t> slots, lengths(S);
  uint32_t longest = 0;
  count_all(*p, lengths.data(), &longest, &slots);
  if (longest > steps) return FX_ERR_CAPACITY;
  const fx::TsOut out{o->hdr, o->dot, o->clock, o->votes, o->nkeys, fx_plane_words(S, steps), steps, 0};
  fx::ts_clear_planes(host_set, out, p->fast_quorum, nullptr);
  if (S) memcpy(o->lengths, lengths.data(), (size_t)S * 4);
  over_items(S, [&](uint32_t t, uint32_t nt) {
    std::vector<uint32_t> state(words);
    for (uint32_t s = t; s < S; s += nt) {
      fx::TsOut mine = out;
      mine.stream = s;
      fx::ts_walk<true>(fx::ts_stream(*p, s), fx::TsWords{state.data(), 1},
                        fx::TsWords{slots.data() + (size_t)s * nslots, 1}, mine);
    }
  });
  return FX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Closed-loop shard groups (fx_table_group_synth.h)
namespace {

struct GroupCounts {
  std::vector<uint32_t> lengths;         // [stream]
  std::vector<uint32_t> rows, lists;     // [group][shard][slot]: cursors (keep_cursors)
  std::vector<uint64_t> list_base;       // [group]
  uint32_t longest = 0, steps_out = 1;
  uint64_t targets_words = 0;
};

// The counting pass of every group.  keep_cursors: rows and lists stay, as
// cursors (the lists' from the group's base in targets, where that fits 32 bits).
void count_groups(const fx_table_group_synth_params& p, bool keep_cursors, GroupCounts& c) {
  const uint32_t Gn = p.groups, P = p.shards, nslots = fx::ts_slots(p), words = fx::tg_state_words(p);
  const size_t per = (size_t)P * nslots;
  c.lengths.assign((size_t)Gn * P, 0u);
  c.list_base.assign(Gn, 0u);
  std::vector<uint32_t> handled((size_t)Gn * P, 0u), total(Gn, 0u);
  if (keep_cursors) {
    c.rows.assign((size_t)Gn * per, 0u);
    c.lists.assign((size_t)Gn * per, 0u);
  }
  over_items(Gn, [&](uint32_t t, uint32_t nt) {
    std::vector<uint32_t> state(words), own_rows(keep_cursors ? 0 : per), own_lists(keep_cursors ? 0 : per), extra(P);
    for (uint32_t g = t; g < Gn; g += nt) {
      uint32_t* r = keep_cursors ? c.rows.data() + g * per : own_rows.data();
      uint32_t* l = keep_cursors ? c.lists.data() + g * per : own_lists.data();
      if (!keep_cursors) {
        std::fill(own_rows.begin(), own_rows.end(), 0u);
        std::fill(own_lists.begin(), own_lists.end(), 0u);
      }
      std::fill(extra.begin(), extra.end(), 0u);
      const fx::TsWords rows{r, 1}, lists{l, 1};
      fx::tg_walk<false>(fx::tg_group(p, g), fx::TsWords{state.data(), 1}, rows, lists, fx::TsWords{extra.data(), 1},
                         fx::TgOut{});
      for (uint32_t h = 0; h < P; ++h) {
        const uint32_t len = fx::ts_prefix(rows.from((size_t)h * nslots), nslots);
        c.lengths[(size_t)g * P + h] = len;
        handled[(size_t)g * P + h] = len + extra[h];
      }
      total[g] = fx::tg_list_words(lists, (uint32_t)per);
    }
  });
  c.longest = 0;
  c.steps_out = 1;
  for (size_t s = 0; s < c.lengths.size(); ++s) {
    c.longest = std::max(c.longest, c.lengths[s]);
    c.steps_out = std::max(c.steps_out, handled[s]);
  }
  c.targets_words = 0;
  for (uint32_t g = 0; g < Gn; ++g) {
    c.list_base[g] = c.targets_words;
    c.targets_words += total[g];
  }
  if (keep_cursors && c.targets_words <= 0xFFFFFFFFull)
    for (uint32_t g = 0; g < Gn; ++g)
      fx::tg_prefix_lists(fx::TsWords{c.lists.data() + g * per, 1}, (uint32_t)per, (uint32_t)c.list_base[g]);
}

bool group_planes_ok(const fx_table_group_synth_planes* o, uint32_t targets_words) {
  return o && o->hdr && o->dot && o->clock && o->votes && o->nkeys && o->route && o->lengths &&
         (o->targets || targets_words == 0);
}

}  // namespace

extern "C" {

int fx_table_group_synth_shape(const fx_table_group_synth_params* p, uint32_t* max_steps, uint32_t* max_steps_out,
                               uint32_t* vmax, uint64_t* max_targets_words) {
  const int st = fx::tg_check(p);
  if (st) return st;
  if (max_steps) *max_steps = (uint32_t)fx::tg_max_rows(*p);
  if (max_steps_out) *max_steps_out = std::max(1u, (uint32_t)fx::tg_max_rows_out(*p));
  if (vmax) *vmax = p->fast_quorum;
  if (max_targets_words) *max_targets_words = fx::tg_max_list_words(*p);
  return FX_OK;
}

size_t fx_table_group_synth_scratch_bytes(const fx_table_group_synth_params* p) {
  if (fx::tg_check(p)) return 0;
  const size_t gpad = ((size_t)p->groups + 63u) / 64u * 64u;
  const uint32_t words = fx::tg_state_words(*p);
  // rows and lists [shard][slot], handled rows [shard], list words and list base, lengths [shard], the state
  return 4u * gpad *
             (2u * (size_t)p->shards * fx::ts_slots(*p) + 2u * p->shards + 2u +
              (words > FX_TABLE_SYNTH_ONCHIP_WORDS ? words : 0u)) +
         16u;
}

int fx_table_group_synth_count_host(const fx_table_group_synth_params* p, uint32_t* lengths, uint32_t* max_len,
                                    uint32_t* steps_out, uint64_t* targets_words) {
  const int st = fx::tg_check(p);
  if (st) return st;
  if (!lengths && p->groups) return FX_ERR_INVALID_ARG;
  GroupCounts c;
  count_groups(*p, false, c);
  if (!c.lengths.empty()) memcpy(lengths, c.lengths.data(), c.lengths.size() * 4);
  if (max_len) *max_len = c.longest;
  if (steps_out) *steps_out = c.steps_out;
  if (targets_words) *targets_words = c.targets_words;
  return FX_OK;
}

int fx_table_group_synth_generate_host(const fx_table_group_synth_params* p, const fx_table_group_synth_planes* o,
                                       uint32_t steps, uint32_t targets_words) {
  const int st = fx::tg_check(p);
  if (st) return st;
  if (!group_planes_ok(o, targets_words)) return FX_ERR_INVALID_ARG;
  const uint32_t Gn = p->groups, P = p->shards, S = Gn * P, words = fx::tg_state_words(*p);
  GroupCounts c;
  count_groups(*p, true, c);
  if (c.longest > steps || c.targets_words > targets_words) return FX_ERR_CAPACITY;
  const fx::TgOut out{{o->hdr, o->dot, o->clock, o->votes, o->nkeys, fx_plane_words(S, steps), steps, 0},
                      o->route, o->targets, targets_words};
  fx::ts_clear_planes(host_set, out.ev, p->fast_quorum, o->route);
  if (S) memcpy(o->lengths, c.lengths.data(), (size_t)S * 4);
  const size_t per = (size_t)P * fx::ts_slots(*p);
  over_items(Gn, [&](uint32_t t, uint32_t nt) {
    std::vector<uint32_t> state(words);
    for (uint32_t g = t; g < Gn; g += nt) {
      fx::TgOut mine = out;
      mine.ev.stream = g * P;
      fx::tg_walk<true>(fx::tg_group(*p, g), fx::TsWords{state.data(), 1}, fx::TsWords{c.rows.data() + g * per, 1},
                        fx::TsWords{c.lists.data() + g * per, 1}, fx::TsWords{nullptr, 1}, mine);
    }
  });
  return FX_OK;
}

}  // extern "C"
