// fx_pending.h — AggregatePending for a batch (host + device): what
// pending_exec.hip and pending_host.cpp share: the count a row carries, the
// word that holds a builder's state, the bucket function of the HBM tier and
// the argument check.
#pragma once
#include <stdint.h>

#include "fx_synth.h"

namespace fx {

// A builder's state word (registers of the ONCHIP tier, entries of the HBM
// tier): 0 = the slot was never used, PENDING_DONE = its command completed,
// else PENDING_LIVE | got << 8 | count.
constexpr uint32_t PENDING_LIVE = 0x80000000u;
constexpr uint32_t PENDING_DONE = 1u;
FX_HD uint32_t pending_word(uint32_t count, uint32_t got) { return PENDING_LIVE | (got << 8) | count; }
FX_HD uint32_t pending_word_count(uint32_t w) { return w & 0xFFu; }
FX_HD uint32_t pending_word_got(uint32_t w) { return (w >> 8) & 0xFFu; }

// The partials the command of a row has, as the stream's owner counts them:
// 0 = nobody here waits for this result.
FX_HD uint32_t pending_count(uint32_t word, uint32_t count_mask, uint32_t rifl, uint32_t process) {
  return process != 0u && (rifl >> 24) != process ? 0u : word & count_mask;
}

FX_HD uint32_t pending_bucket(uint32_t rifl, uint32_t buckets) {
  uint32_t x = rifl * 0x9E3779B1u;
  x ^= x >> 15;
  return x % buckets;
}
FX_HD uint32_t pending_buckets(uint32_t steps) { return steps < 64u ? 1u : (steps + 63u) / 64u; }

inline int pending_check(const fx_pending_batch* in, const fx_pending_out* out, uint32_t tier) {
  if (!in || !out || !in->order || !in->nexec || !in->rifl || !in->count || !out->part || !out->head || !out->ready ||
      !out->index || !out->nready || !out->nopen || !out->err)
    return FX_ERR_INVALID_ARG;
  if (in->count_mask == 0u || tier > FX_PENDING_TIER_HBM) return FX_ERR_INVALID_ARG;
  return FX_OK;
}

}  // namespace fx
