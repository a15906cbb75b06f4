// slot_host.cpp — the host twins of slot_exec.hip and slot_advance.hip
// (fx_slot_execute_host, fx_slot_advance_host, fx_slot_synth_generate_host) and
// the functions of the engine that need no device, fx_slot_state_bytes and
// fx_slot_session_bytes (fx_slot.h holds what the two sides share).
// No HIP call in here, so the file also builds alone with a host compiler
// (tests/cpp/slot_host_check.cpp, slot_advance_host_check.cpp under the
// sanitizers).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the function attributes of fx_synth.h
#endif
#include <vector>

#include "fx_slot.h"

extern "C" {

// the SCAN tier's table: the arrival row of every slot 1 .. steps, the rows of a
// lane's table rounded up to a whole 256-byte line
size_t fx_slot_state_bytes(uint32_t steps, uint32_t lanes) {
  return (size_t)lanes * (((size_t)steps + 63u) & ~(size_t)63u) * 4u;
}

int fx_slot_execute_host(const fx_slot_batch* inp, const fx_order_batch* out, uint32_t flags) {
  const int st = fx::slot_check(inp, out, flags);
  if (st) return st;
  const fx_slot_batch& in = *inp;
  const uint32_t steps = in.steps;
  const bool at_commit = (flags & FX_FLAG_EXECUTE_AT_COMMIT) != 0u;
  std::vector<uint32_t> row_of;  // by slot - 1: its arrival row while it waits, else FX_RELEASE_NONE
  for (uint32_t s = 0; s < in.num_streams; ++s) {
    const uint32_t len = fx::slot_length(in.lengths, s, steps);
    uint32_t next = 1, nexec = 0, status = FX_OK;
    row_of.assign(steps, FX_RELEASE_NONE);
    for (uint32_t a = 0; a < len && !status; ++a) {
      const uint32_t slot = in.slot[fx_index(a, s, steps)];
      if (at_commit) {
        if (slot == 0u) {
          status = FX_ERR_SLOT;
          break;
        }
        out->order[fx_index(nexec++, s, steps)] = a | FX_ORDER_SCC_START;
        out->release[fx_index(a, s, steps)] = a;
        continue;
      }
      status = fx::slot_row_status(slot, next, steps, 0u);
      if (!status && row_of[slot - 1u] != FX_RELEASE_NONE) status = FX_ERR_SLOT;
      if (status) break;
      row_of[slot - 1u] = a;
      if (slot != next) out->release[fx_index(a, s, steps)] = FX_RELEASE_NONE;
      while (next <= steps && row_of[next - 1u] != FX_RELEASE_NONE) {
        const uint32_t r = row_of[next - 1u];
        row_of[next - 1u] = FX_RELEASE_NONE;
        out->order[fx_index(nexec++, s, steps)] = r | FX_ORDER_SCC_START;
        out->release[fx_index(r, s, steps)] = a;
        ++next;
      }
    }
    out->nexec[s] = nexec;
    out->err[s] = status;
  }
  return FX_OK;
}

size_t fx_slot_session_bytes(uint32_t steps, uint32_t num_streams) {
  return (size_t)num_streams * fx::slot_session_stride(steps) * 4u;
}

// The sequential executor over the session's state (fx_slot.h): T keeps the
// arrival row of every slot that arrived, executed ones included, so `a slot
// that arrived` is one look-up; next = E + 1.  A stopped stream's T differs
// from the device's (which has seen the rows behind the failing one), and
// neither is read again.
int fx_slot_advance_host(const fx_slot_batch* inp, const fx_order_batch* out, void* state, uint32_t flags) {
  const int st = fx::slot_advance_check(inp, out, state, flags);
  if (st) return st;
  const fx_slot_batch& in = *inp;
  const uint32_t steps = in.steps;
  if (in.num_streams == 0u || steps == 0u) return FX_OK;
  const bool at_commit = (flags & FX_FLAG_EXECUTE_AT_COMMIT) != 0u;
  for (uint32_t s = 0; s < in.num_streams; ++s) {
    uint32_t* const H = (uint32_t*)state + (size_t)s * fx::slot_session_stride(steps);
    uint32_t* const T = H + fx::SLOT_H_WORDS;
    const uint32_t len = fx::slot_length(in.lengths, s, steps);
    uint32_t done = 0, E = 0, carry = 0, status = FX_OK;
    if (flags & FX_FLAG_INIT) {
      for (uint32_t i = 0; i < steps; ++i) T[i] = FX_RELEASE_NONE;
    } else {
      done = H[fx::SLOT_H_DONE], E = H[fx::SLOT_H_E], carry = H[fx::SLOT_H_CARRY], status = H[fx::SLOT_H_ERR];
      if (!fx::slot_header_ok(H[fx::SLOT_H_TAG], H[fx::SLOT_H_STEPS], done, E, steps, at_commit)) {
        out->err[s] = FX_ERR_INVALID_ARG;
        continue;
      }
      if (!status && len < done) {
        out->err[s] = FX_ERR_INVALID_ARG;
        continue;
      }
      if (status || len == done) {
        out->nexec[s] = E;
        out->err[s] = status;
        continue;
      }
    }
    for (uint32_t a = done; a < len && !status; ++a) {
      const uint32_t slot = in.slot[fx_index(a, s, steps)];
      if (at_commit) {
        if (slot == 0u) {
          status = FX_ERR_SLOT;
          break;
        }
        out->order[fx_index(E++, s, steps)] = a | FX_ORDER_SCC_START;
        out->release[fx_index(a, s, steps)] = a;
        continue;
      }
      status = fx::slot_row_status(slot, E + 1u, steps, 0u);
      if (!status && T[slot - 1u] != FX_RELEASE_NONE) status = FX_ERR_SLOT;
      if (status) break;
      T[slot - 1u] = a;
      if (slot != E + 1u) out->release[fx_index(a, s, steps)] = FX_RELEASE_NONE;
      while (E < steps && T[E] != FX_RELEASE_NONE) {
        out->order[fx_index(E, s, steps)] = T[E] | FX_ORDER_SCC_START;
        out->release[fx_index(T[E], s, steps)] = a;
        carry = a;
        ++E;
      }
    }
    H[fx::SLOT_H_TAG] = fx::SLOT_TAG | (at_commit ? 1u : 0u);
    H[fx::SLOT_H_STEPS] = steps;
    H[fx::SLOT_H_DONE] = len;
    H[fx::SLOT_H_E] = E;
    H[fx::SLOT_H_CARRY] = carry;
    H[fx::SLOT_H_ERR] = status;
    out->nexec[s] = E;
    out->err[s] = status;
  }
  return FX_OK;
}

int fx_slot_synth_generate_host(uint64_t seed, uint32_t stream_base, uint32_t num_streams, uint32_t steps,
                                const uint32_t* lengths, uint32_t window, uint32_t* slot_plane) {
  const int st = fx::slot_synth_check(stream_base, num_streams, steps, window, slot_plane);
  if (st) return st;
  const size_t plane = fx_plane_words(num_streams, steps);
  for (size_t w = 0; w < plane; ++w) {
    uint32_t s = 0, slot = 0, row = 0;
    if (fx::slot_synth_word(w, seed, stream_base, lengths, num_streams, steps, window, &s, &slot, &row))
      slot_plane[fx_index(row, s, steps)] = slot;
    else
      slot_plane[w] = 0u;
  }
  return FX_OK;
}

}  // extern "C"
