// pending_host.cpp — the host twin of pending_exec.hip
// (fx_pending_aggregate_host), and the two functions of the stage that need no
// device: fx_pending_bucket, fx_pending_state_bytes (fx_pending.h holds what
// the two sides share).  No HIP call in here, so the file also builds alone
// with a host compiler (tests/cpp/pending_host_check.cpp under the sanitizers).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the function attributes of fx_synth.h
#endif
#include <unordered_map>

#include "fx_pending.h"

namespace {

struct Builder {
  uint32_t head, count, got;
};

}  // namespace

extern "C" {

uint32_t fx_pending_bucket(uint32_t rifl, uint32_t buckets) { return buckets ? fx::pending_bucket(rifl, buckets) : 0u; }

size_t fx_pending_state_bytes(uint32_t steps, uint32_t lanes) {
  return (size_t)lanes * fx::pending_buckets(steps) * 64u * 16u;
}

int fx_pending_aggregate_host(const fx_pending_batch* inp, const fx_pending_out* out, uint32_t tier) {
  const int st = fx::pending_check(inp, out, tier);
  if (st) return st;
  const fx_pending_batch& in = *inp;
  const size_t plane = fx_plane_words(in.num_streams, in.steps);
  for (uint32_t s = 0; s < in.num_streams; ++s) {
    const uint32_t ne = in.nexec[s];
    uint32_t nready = 0, status = FX_OK;
    std::unordered_map<uint32_t, Builder> live;
    if (ne > in.steps) status = FX_ERR_ORDER_OVERFLOW;
    for (uint32_t k = 0; k < ne && !status; ++k) {
      const uint32_t a = FX_ORDER_REC(in.order[fx_index(k, s, in.steps)]);
      if (a >= in.steps) {
        status = FX_ERR_INVALID_ARG;
        break;
      }
      const size_t at = fx_index(a, s, in.steps);
      const uint32_t r = in.rifl[at], c = fx::pending_count(in.count[at], in.count_mask, r, in.process);
      if (c == 0u) {
        out->head[at] = FX_PENDING_IGNORED;
        continue;
      }
      if (c > FX_PENDING_MAX_PARTS) {
        status = FX_ERR_INVALID_ARG;
        break;
      }
      uint32_t head = a, slot = 0;
      bool completes = true;
      if (c > 1u) {
        auto it = live.find(r);
        if (it == live.end()) {
          if (tier == FX_PENDING_TIER_ONCHIP && live.size() >= FX_PENDING_ONCHIP_LIVE) {
            status = FX_ERR_CAPACITY;
            break;
          }
          it = live.emplace(r, Builder{a, c, 0u}).first;
        } else if (it->second.count != c) {
          status = FX_ERR_INVALID_ARG;
          break;
        }
        head = it->second.head;
        slot = it->second.got++;
        completes = it->second.got == c;
        if (completes) live.erase(it);
      }
      const size_t hat = fx_index(head, s, in.steps);
      out->part[slot * plane + hat] = a;
      out->head[at] = head;
      if (completes) {
        out->index[hat] = nready;
        out->ready[fx_index(nready, s, in.steps)] = head;
        ++nready;
      }
    }
    out->nready[s] = nready;
    out->nopen[s] = (uint32_t)live.size();
    out->err[s] = status;
  }
  return FX_OK;
}

}  // extern "C"
