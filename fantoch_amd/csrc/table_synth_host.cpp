// table_synth_host.cpp — the host side of the synthetic Tempo vote streams
// (fx_table_synth.h): argument checks, the shape, and the host twin of the
// generator.  No HIP call in here, so the file also builds alone with a host
// compiler (tests/cpp/table_synth_host_check.cpp under the sanitizers).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the function attributes of fx_synth.h
#endif
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "fx_table_synth.h"

namespace {

// The counting pass of every stream: lengths[s], and the longest.  slots_out
// (optional): the first rows of every stream's slots, [stream][slot].
void count_all(const fx_table_synth_params& p, uint32_t* lengths, uint32_t* max_len,
               std::vector<uint32_t>* slots_out) {
  const uint32_t S = p.streams, nslots = fx::ts_slots(p), words = fx::ts_state_words(p);
  if (slots_out) slots_out->assign((size_t)S * nslots, 0u);
  const uint32_t nt = S < 64 ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<uint32_t> longest(nt, 0u);
  auto work = [&](uint32_t t) {
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
  };
  std::vector<std::thread> th;
  for (uint32_t t = 1; t < nt; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
  if (max_len) *max_len = *std::max_element(longest.begin(), longest.end());
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
  const size_t plane = fx_plane_words(S, steps);
  memset(o->hdr, 0, plane * 4);
  memset(o->dot, 0, plane * 4);
  memset(o->clock, 0, plane * 4);
  memset(o->votes, 0, plane * 4 * 3 * p->fast_quorum);
  if (o->nkeys) memset(o->nkeys, 0, plane * 4);
  if (S) memcpy(o->lengths, lengths.data(), (size_t)S * 4);
  // every stream writes its own words of the planes: streams split over threads
  const uint32_t nt = S < 64 ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  auto work = [&](uint32_t t) {
    std::vector<uint32_t> state(words);
    for (uint32_t s = t; s < S; s += nt) {
      const fx::TsOut out{o->hdr, o->dot, o->clock, o->votes, o->nkeys, plane, steps, s};
      fx::ts_walk<true>(fx::ts_stream(*p, s), fx::TsWords{state.data(), 1},
                        fx::TsWords{slots.data() + (size_t)s * nslots, 1}, out);
    }
  };
  std::vector<std::thread> th;
  for (uint32_t t = 1; t < nt; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
  return FX_OK;
}

}  // extern "C"
