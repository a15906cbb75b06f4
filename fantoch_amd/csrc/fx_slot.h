// fx_slot.h — the slot executor (FPaxos) for a batch (host + device): what
// slot_exec.hip and slot_host.cpp share: the argument checks, what a row's
// slot means to an executor, and the generator's key and row functions.
#pragma once
#include <stdint.h>

#include "fx_synth.h"

namespace fx {

// purpose of the generator's draw (the last argument of synth_rand; the ones in
// use: fx_kv.h)
enum : uint64_t { SLOT_DRAW = 17 };

// A row with slot s at an executor whose next slot is `next`, before its
// waiting set is looked at: FX_ERR_SLOT for a slot that is 0 or was executed,
// FX_ERR_CAPACITY for one the tables cannot hold (above `steps`, or `window`
// != 0 and s - next >= window), else FX_OK: the slot waits, unless it already
// does (FX_ERR_SLOT, the caller's look-up).
FX_HD uint32_t slot_row_status(uint32_t s, uint32_t next, uint32_t steps, uint32_t window) {
  if (s < next) return FX_ERR_SLOT;
  if (s > steps || (window != 0u && s - next >= window)) return FX_ERR_CAPACITY;
  return FX_OK;
}

FX_HD uint32_t slot_length(const uint32_t* lengths, uint32_t s, uint32_t steps) {
  const uint32_t len = lengths ? lengths[s] : steps;
  return len < steps ? len : steps;
}

inline int slot_check(const fx_slot_batch* in, const fx_order_batch* out, uint32_t flags) {
  if (!in || !out || !in->slot || !out->order || !out->release || !out->nexec || !out->err) return FX_ERR_INVALID_ARG;
  if (in->steps >= (1u << 31) || (flags & ~FX_FLAG_EXECUTE_AT_COMMIT) != 0u) return FX_ERR_INVALID_ARG;
  return FX_OK;
}

// Sessions (fx_slot_advance): per stream a header of SLOT_H_WORDS words, then
// T[slot - 1] = the first arrival row of the slot (FX_RELEASE_NONE: none yet),
// `steps` words rounded up to a whole 256-byte line.  SLOT_H_E = the executed
// slots (next - 1; at commit the executed rows), SLOT_H_CARRY = the release
// step of the last of them, SLOT_H_ERR = the status the stream stopped with.
enum : uint32_t { SLOT_H_TAG = 0, SLOT_H_STEPS = 1, SLOT_H_DONE = 2, SLOT_H_E = 3, SLOT_H_CARRY = 4, SLOT_H_ERR = 5,
                  SLOT_H_WORDS = 64 };
constexpr uint32_t SLOT_TAG = 0x534C4F54u;  // "SLOT"; bit 0: the session executes at commit

FX_HD size_t slot_session_stride(uint32_t steps) { return (size_t)SLOT_H_WORDS + (((size_t)steps + 63u) & ~(size_t)63u); }

inline int slot_advance_check(const fx_slot_batch* in, const fx_order_batch* out, const void* state, uint32_t flags) {
  if (!state || (flags & ~(FX_FLAG_INIT | FX_FLAG_EXECUTE_AT_COMMIT)) != 0u) return FX_ERR_INVALID_ARG;
  return slot_check(in, out, flags & FX_FLAG_EXECUTE_AT_COMMIT);
}

// A header a call may continue from: written by a call with FX_FLAG_INIT and
// the same steps and commit flag, and no index in it beyond what it indexes.
FX_HD bool slot_header_ok(uint32_t tag, uint32_t hsteps, uint32_t done, uint32_t E, uint32_t steps, bool at_commit) {
  return tag == (SLOT_TAG | (at_commit ? 1u : 0u)) && hsteps == steps && done <= steps && E <= done;
}

inline int slot_synth_check(uint32_t stream_base, uint32_t num_streams, uint32_t steps, uint32_t window,
                            const uint32_t* slot_plane) {
  if (!slot_plane || window == 0u || steps >= (1u << 31) || (uint64_t)stream_base + num_streams > (1ull << 32))
    return FX_ERR_INVALID_ARG;
  return FX_OK;
}

// The key of slot s of global stream g: the arrival order of a stream is its
// slots sorted by (key, slot).
FX_HD uint64_t slot_synth_key(uint64_t seed, uint64_t g, uint32_t s, uint32_t window) {
  return (uint64_t)s + synth_rand(seed, g, s, SLOT_DRAW) % window;
}

// The arrival row of slot s (1 .. L) of global stream g: the slots before it
// in that order.  Every slot at or below s - window is (key <= its slot +
// window - 1 < s), none at or above s + window is.
FX_HD uint32_t slot_synth_row(uint64_t seed, uint64_t g, uint32_t s, uint32_t L, uint32_t window) {
  const uint64_t key = slot_synth_key(seed, g, s, window);
  const uint32_t lo = s > window ? s - window + 1u : 1u;
  const uint32_t hi = L - s < window ? L : s + window - 1u;
  uint32_t row = lo - 1u;
  for (uint32_t o = lo; o <= hi; ++o) {
    if (o == s) continue;
    const uint64_t k = slot_synth_key(seed, g, o, window);
    row += (k < key || (k == key && o < s)) ? 1u : 0u;
  }
  return row;
}

// Word w of a plane of (S, steps), seen as (stream, i): the arrival row that
// slot i + 1 of the stream lands on and true, or false for a word that holds
// no slot (a pad word, a row past the stream's length), which is 0 where it is.
FX_HD bool slot_synth_word(size_t w, uint64_t seed, uint32_t stream_base, const uint32_t* lengths, uint32_t S,
                           uint32_t steps, uint32_t window, uint32_t* stream, uint32_t* slot, uint32_t* row) {
  const size_t tile = w >> 8, steps4 = (steps + 3u) >> 2;
  const uint32_t s = (uint32_t)(tile / steps4) * 64u + (uint32_t)((w >> 2) & 63u);
  const uint32_t i = (uint32_t)(tile % steps4) * 4u + (uint32_t)(w & 3u);
  if (s >= S || i >= steps) return false;
  const uint32_t L = slot_length(lengths, s, steps);
  if (i >= L) return false;
  *stream = s;
  *slot = i + 1u;
  *row = slot_synth_row(seed, (uint64_t)stream_base + s, i + 1u, L, window);
  return true;
}

}  // namespace fx
