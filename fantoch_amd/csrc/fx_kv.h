// fx_kv.h — KVStore semantics of one partial and the op generator (host +
// device): what kv_exec.hip and kv_advance.hip run per lane (kv_step.inc) and
// kv_host.cpp per row, and the state layout, the checks and the header write of
// the sessions (fx_kv_advance).
//
// A partial is up to omax op words on one key (kvs.rs:53-85).  Its effect on
// the key splits in two: what it leaves behind does not depend on what it
// found (the last Put's value, or nothing after a last Delete), and only its
// results do.  kv_fold gives the first half, kv_walk the second.
#pragma once
#include <stdint.h>

#include "fx_synth.h"

namespace fx {

// purpose of the op draw (the last argument of synth_rand; fx_synth.h uses
// 1 .. 4 and 10, fx_table_synth.h 32 .. 36, 40 .. 63 and 128 .. 255,
// fx_table_group_synth.h 37, 38 and 64 .. 127)
enum : uint64_t { KV_OP_DRAW = 16 };
constexpr uint32_t KV_VALUES = 0x3FFFFFFFu;  // values 1 .. 2^30 - 1

struct KvFold {
  bool writes;      // some op is a Put or a Delete
  bool bad;         // a Put of value 0, or a used slot after an EMPTY one
  uint32_t leaves;  // writes only: the key's value afterwards, 0 = absent
};

FX_HD KvFold kv_fold(const uint32_t (&op)[FX_KV_MAX_OPS], uint32_t omax) {
  KvFold f{false, false, 0u};
  bool ended = false;
#pragma unroll
  for (uint32_t j = 0; j < FX_KV_MAX_OPS; ++j)
    if (j < omax) {
      const uint32_t kind = FX_KV_OP_KIND(op[j]), v = FX_KV_OP_VALUE(op[j]);
      if (kind == FX_KV_EMPTY) {
        ended = true;
        continue;
      }
      f.bad |= ended || (kind == FX_KV_PUT && v == 0u);
      if (kind != FX_KV_GET) {
        f.writes = true;
        f.leaves = kind == FX_KV_PUT ? v : 0u;
      }
    }
  return f;
}

// Results of the slots given the value the partial found (kvs.rs:74-84).
FX_HD void kv_walk(const uint32_t (&op)[FX_KV_MAX_OPS], uint32_t omax, uint32_t found,
                   uint32_t (&res)[FX_KV_MAX_OPS]) {
  uint32_t cur = found;
#pragma unroll
  for (uint32_t j = 0; j < FX_KV_MAX_OPS; ++j) {
    res[j] = 0u;
    if (j < omax) {
      const uint32_t kind = FX_KV_OP_KIND(op[j]);
      if (kind == FX_KV_GET || kind == FX_KV_DELETE) res[j] = cur;
      if (kind == FX_KV_PUT) cur = FX_KV_OP_VALUE(op[j]);
      if (kind == FX_KV_DELETE) cur = 0u;
    }
  }
}

inline int kv_check(const fx_kv_batch* in, const fx_kv_out* out) {
  if (!in || !out || !in->order || !in->nexec || !in->key || !in->ops || !out->result || !out->store ||
      !out->monitor || !out->mon_off || !out->err)
    return FX_ERR_INVALID_ARG;
  if (in->omax < 1 || in->omax > FX_KV_MAX_OPS || in->keys < 1 || in->keys > FX_TABLE_MAX_KEYS)
    return FX_ERR_INVALID_ARG;
  return FX_OK;
}

// Sessions (fx_kv_advance): per stream a header of KV_H_WORDS words, then the
// value of every key and the write partials executed on every key so far, each
// `keys` words rounded up to a whole 256-byte line.  Entry k of either table
// belongs to lane k & 63.  KV_H_DONE = the order rows consumed, KV_H_ERR = the
// status the stream stopped with.
enum : uint32_t { KV_H_TAG = 0, KV_H_STEPS = 1, KV_H_KEYS = 2, KV_H_OMAX = 3, KV_H_DONE = 4, KV_H_ERR = 5,
                  KV_H_WORDS = 64 };
constexpr uint32_t KV_TAG = 0x4B565353u;  // "KVSS"

FX_HD size_t kv_session_keys(uint32_t keys) { return ((size_t)keys + 63u) & ~(size_t)63u; }
FX_HD size_t kv_session_stride(uint32_t keys) { return (size_t)KV_H_WORDS + 2u * kv_session_keys(keys); }

// A header a call may continue from: written by a call with FX_FLAG_INIT and
// the same steps, keys and omax, and no index in it beyond what it indexes.
FX_HD bool kv_header_ok(uint32_t tag, uint32_t hsteps, uint32_t hkeys, uint32_t homax, uint32_t done, uint32_t steps,
                        uint32_t keys, uint32_t omax) {
  return tag == KV_TAG && hsteps == steps && hkeys == keys && homax == omax && done <= steps;
}

// The header as a call leaves it (by lane 0 on the device).
FX_HD void kv_write_header(uint32_t* H, uint32_t steps, uint32_t keys, uint32_t omax, uint32_t done, uint32_t err) {
  H[KV_H_TAG] = KV_TAG, H[KV_H_STEPS] = steps, H[KV_H_KEYS] = keys, H[KV_H_OMAX] = omax;
  H[KV_H_DONE] = done, H[KV_H_ERR] = err;
}

inline int kv_batch_check(const fx_kv_batch* in) {
  if (!in || !in->order || !in->nexec || !in->key || !in->ops) return FX_ERR_INVALID_ARG;
  if (in->omax < 1 || in->omax > FX_KV_MAX_OPS || in->keys < 1 || in->keys > FX_TABLE_MAX_KEYS)
    return FX_ERR_INVALID_ARG;
  return FX_OK;
}

inline int kv_advance_check(const fx_kv_batch* in, const fx_kv_session_out* out, const void* state, uint32_t flags) {
  if (!out || !out->result || !out->store || !out->rank || !out->err || !state || (flags & ~FX_FLAG_INIT) != 0u)
    return FX_ERR_INVALID_ARG;
  return kv_batch_check(in);
}

inline int kv_session_monitor_check(const fx_kv_batch* in, const uint32_t* rank, const fx_kv_out* out,
                                    const void* state) {
  if (!rank || !state) return FX_ERR_INVALID_ARG;
  return kv_check(in, out);
}

inline int kv_monitor_check(const fx_kv_monitor* a, const fx_kv_monitor* b, const uint32_t* pairs, uint32_t num_pairs,
                            const uint32_t* diff) {
  if (!a || !b || !a->monitor || !a->mon_off || !a->rifl || !b->monitor || !b->mon_off || !b->rifl)
    return FX_ERR_INVALID_ARG;
  if (num_pairs && (!pairs || !diff)) return FX_ERR_INVALID_ARG;
  if (a->keys < 1 || a->keys > FX_TABLE_MAX_KEYS || a->keys != b->keys) return FX_ERR_INVALID_ARG;
  return FX_OK;
}

inline int kv_synth_check(uint32_t stream_base, uint32_t read_pct, uint32_t delete_pct, uint32_t num_streams,
                          const uint32_t* ops) {
  if (!ops || read_pct > 100 || delete_pct > 100 || read_pct + delete_pct > 100 ||
      (uint64_t)stream_base + num_streams > (1ull << 32))
    return FX_ERR_INVALID_ARG;
  return FX_OK;
}

FX_HD uint32_t kv_synth_op(uint64_t seed, uint64_t g, uint32_t row, uint32_t read_pct, uint32_t delete_pct) {
  const uint64_t d = synth_rand(seed, g, row, KV_OP_DRAW);
  const uint32_t p = (uint32_t)((d >> 32) % 100u);
  if (p < read_pct) return FX_KV_OP(FX_KV_GET, 0u);
  if (p < read_pct + delete_pct) return FX_KV_OP(FX_KV_DELETE, 0u);
  return FX_KV_OP(FX_KV_PUT, 1u + (uint32_t)(d % KV_VALUES));
}

// Word w of a plane of (S, steps): its op.  Pad words (a stream >= S, a step
// >= steps) and rows at or past the stream's length are EMPTY.
FX_HD uint32_t kv_synth_word(size_t w, uint64_t seed, uint32_t stream_base, uint32_t read_pct, uint32_t delete_pct,
                             const uint32_t* lengths, uint32_t S, uint32_t steps) {
  const size_t tile = w >> 8, steps4 = (steps + 3u) >> 2;
  const uint32_t s = (uint32_t)(tile / steps4) * 64u + (uint32_t)((w >> 2) & 63u);
  const uint32_t row = (uint32_t)(tile % steps4) * 4u + (uint32_t)(w & 3u);
  if (s >= S || row >= steps || (lengths && row >= lengths[s])) return FX_KV_OP(FX_KV_EMPTY, 0u);
  return kv_synth_op(seed, (uint64_t)stream_base + s, row, read_pct, delete_pct);
}

}  // namespace fx
