// pending_host.cpp — the host twins of pending_exec.hip and pending_advance.hip
// (fx_pending_aggregate_host, fx_pending_advance_host), and the functions of
// the stage that need no device: fx_pending_bucket, fx_pending_state_bytes,
// fx_pending_session_bytes (fx_pending.h holds what the two sides share).  No
// HIP call in here, so the file also builds alone with a host compiler
// (tests/cpp/pending_host_check.cpp, pending_advance_host_check.cpp under the
// sanitizers).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the function attributes of fx_synth.h
#endif
#include <unordered_map>

#include "fx_pending.h"

namespace {

struct Builder {
  uint32_t head, count, got;
};

// Order row k of stream s against the live builders: FX_OK, or the status the
// stream stops with at this row, nothing of which is stored.  max_live: the
// builders the tier holds.
uint32_t pending_row(const fx_pending_batch& in, const fx_pending_out* out, size_t plane, uint32_t s, uint32_t k,
                     std::unordered_map<uint32_t, Builder>& live, size_t max_live, uint32_t& nready) {
  const uint32_t a = FX_ORDER_REC(in.order[fx_index(k, s, in.steps)]);
  if (a >= in.steps) return FX_ERR_INVALID_ARG;
  const size_t at = fx_index(a, s, in.steps);
  const uint32_t r = in.rifl[at], c = fx::pending_count(in.count[at], in.count_mask, r, in.process);
  if (c == 0u) {
    out->head[at] = FX_PENDING_IGNORED;
    return FX_OK;
  }
  if (c > FX_PENDING_MAX_PARTS) return FX_ERR_INVALID_ARG;
  uint32_t head = a, slot = 0;
  bool completes = true;
  if (c > 1u) {
    auto it = live.find(r);
    if (it == live.end()) {
      if (live.size() >= max_live) return FX_ERR_CAPACITY;
      it = live.emplace(r, Builder{a, c, 0u}).first;
    } else if (it->second.count != c) {
      return FX_ERR_INVALID_ARG;
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
  return FX_OK;
}

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
    const size_t max_live = tier == FX_PENDING_TIER_ONCHIP ? (size_t)FX_PENDING_ONCHIP_LIVE : SIZE_MAX;
    for (uint32_t k = 0; k < ne && !status; ++k) status = pending_row(in, out, plane, s, k, live, max_live, nready);
    out->nready[s] = nready;
    out->nopen[s] = (uint32_t)live.size();
    out->err[s] = status;
  }
  return FX_OK;
}

size_t fx_pending_session_bytes(uint32_t steps, uint32_t num_streams) {
  return (size_t)num_streams * fx::pending_session_stride(steps) * 4u;
}

// The sequential stage over a session's state (fx_pending.h).  Between calls
// the live builders are packed into the table's entries from 0 on; a builder
// is created by an order row of its own, so there are never more than the
// table's entries.  The state is this side's own: only the outputs are the
// device's bytes.
int fx_pending_advance_host(const fx_pending_batch* inp, const fx_pending_out* out, void* state, uint32_t flags) {
  const int st = fx::pending_advance_check(inp, out, state, flags);
  if (st) return st;
  const fx_pending_batch& in = *inp;
  const size_t plane = fx_plane_words(in.num_streams, in.steps);
  const uint32_t steps = in.steps;
  const size_t entries = (size_t)fx::pending_buckets(steps) * 64u;
  for (uint32_t s = 0; s < in.num_streams; ++s) {
    uint32_t* const H = (uint32_t*)state + (size_t)s * fx::pending_session_stride(steps);
    uint32_t* const tab = H + fx::PENDING_H_WORDS;
    const uint32_t ne = in.nexec[s];
    uint32_t done = 0, nready = 0, status = FX_OK;
    std::unordered_map<uint32_t, Builder> live;
    if (!(flags & FX_FLAG_INIT)) {
      uint32_t h[8];
      for (uint32_t i = 0; i < 8u; ++i) h[i] = H[i];
      if (!fx::pending_header_ok(h, steps, in.count_mask, in.process)) {
        out->err[s] = FX_ERR_INVALID_ARG;
        continue;
      }
      done = h[fx::PENDING_H_DONE], nready = h[fx::PENDING_H_NREADY], status = h[fx::PENDING_H_ERR];
      if (status || ne > steps || ne <= done) {
        out->err[s] = status ? status : ne > steps ? FX_ERR_ORDER_OVERFLOW : ne < done ? FX_ERR_INVALID_ARG : FX_OK;
        continue;
      }
      // entries whose count or head row is not what a session writes are no builders, as on the device
      for (size_t i = 0; i < h[fx::PENDING_H_LIVE] && i < entries; ++i) {
        const uint32_t* e = tab + 4u * i;
        const uint32_t c = fx::pending_word_count(e[2]);
        if ((e[2] & fx::PENDING_LIVE) && e[1] < steps && c >= 2u && c <= FX_PENDING_MAX_PARTS)
          live.emplace(e[0], Builder{e[1], c, fx::pending_word_got(e[2])});
      }
    }
    const uint32_t end = ne > steps ? 0u : ne;
    for (uint32_t k = done; k < end && !status; ++k) status = pending_row(in, out, plane, s, k, live, SIZE_MAX, nready);
    size_t i = 0;
    for (const auto& b : live) {
      if (i == entries) break;  // not reached: a builder per creating order row at most
      uint32_t* e = tab + 4u * i++;
      e[0] = b.first, e[1] = b.second.head, e[2] = fx::pending_word(b.second.count, b.second.got), e[3] = 0u;
    }
    fx::pending_write_header(H, steps, in.count_mask, in.process, end, nready, (uint32_t)live.size(), status);
    out->nready[s] = nready;
    out->nopen[s] = (uint32_t)live.size();
    out->err[s] = ne > steps ? FX_ERR_ORDER_OVERFLOW : status;
  }
  return FX_OK;
}

}  // extern "C"
