// fx_pending.h — AggregatePending for a batch (host + device): what
// the kernels (pending_exec.hip, pending_advance.hip; their chunk step:
// pending_step.inc) and pending_host.cpp share: the count a row carries, the
// word that holds a builder's state, the bucket function of the HBM tier and
// the argument check; for the sessions: the state layout, the header check and
// the header write.
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

// Sessions (fx_pending_advance): per stream a header of PENDING_H_WORDS words,
// then the table: pending_buckets(steps) buckets of 64 entries of 16 bytes
// (the device: the HBM tier's table; the host twin: its live builders, packed
// from entry 0 on, as {rifl, head row, pending_word(count, got), 0}).
// PENDING_H_DONE = the order rows consumed, PENDING_H_NREADY / PENDING_H_LIVE =
// the completed commands and the live builders so far, PENDING_H_ERR = the
// status the stream stopped with.
enum : uint32_t { PENDING_H_TAG = 0, PENDING_H_STEPS = 1, PENDING_H_MASK = 2, PENDING_H_PROCESS = 3,
                  PENDING_H_DONE = 4, PENDING_H_NREADY = 5, PENDING_H_LIVE = 6, PENDING_H_ERR = 7,
                  PENDING_H_WORDS = 64 };
constexpr uint32_t PENDING_TAG = 0x50454E44u;  // "PEND"

FX_HD size_t pending_session_stride(uint32_t steps) {
  return (size_t)PENDING_H_WORDS + (size_t)pending_buckets(steps) * 64u * 4u;
}

// A header a call may continue from: written by a call with FX_FLAG_INIT and
// the same steps, count_mask and process, and no count in it beyond the rows
// that can have produced it.
FX_HD bool pending_header_ok(const uint32_t (&h)[8], uint32_t steps, uint32_t count_mask, uint32_t process) {
  return h[PENDING_H_TAG] == PENDING_TAG && h[PENDING_H_STEPS] == steps && h[PENDING_H_MASK] == count_mask &&
         h[PENDING_H_PROCESS] == process && h[PENDING_H_DONE] <= steps && h[PENDING_H_NREADY] <= h[PENDING_H_DONE] &&
         h[PENDING_H_LIVE] <= h[PENDING_H_DONE];
}

// The header as a call leaves it (by lane 0 on the device).
FX_HD void pending_write_header(uint32_t* H, uint32_t steps, uint32_t count_mask, uint32_t process, uint32_t done,
                                uint32_t nready, uint32_t live, uint32_t err) {
  H[PENDING_H_TAG] = PENDING_TAG, H[PENDING_H_STEPS] = steps;
  H[PENDING_H_MASK] = count_mask, H[PENDING_H_PROCESS] = process;
  H[PENDING_H_DONE] = done, H[PENDING_H_NREADY] = nready, H[PENDING_H_LIVE] = live;
  H[PENDING_H_ERR] = err;
}

inline int pending_advance_check(const fx_pending_batch* in, const fx_pending_out* out, const void* state,
                                 uint32_t flags) {
  if (!state || (flags & ~FX_FLAG_INIT) != 0u) return FX_ERR_INVALID_ARG;
  return pending_check(in, out, FX_PENDING_TIER_HBM);
}

}  // namespace fx
