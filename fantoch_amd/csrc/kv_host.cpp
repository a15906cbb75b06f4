// kv_host.cpp — the host twins of kv_exec.hip and kv_advance.hip:
// fx_kv_execute_host, fx_kv_monitor_compare_host, fx_kv_synth_ops_host,
// fx_kv_advance_host, fx_kv_session_monitor_host, and fx_kv_session_bytes,
// which needs no device (fx_kv.h holds what the two sides share).  No HIP call
// in here, so the file also builds alone with a host compiler
// (tests/cpp/kv_host_check.cpp, kv_advance_host_check.cpp under the sanitizers).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the function attributes of fx_synth.h
#endif
#include <algorithm>
#include <vector>

#include "fx_kv.h"

namespace {

struct Row {
  uint32_t a, key;
  uint32_t op[FX_KV_MAX_OPS];
};

// Row k of stream s's order; false: the arrival row or the key is out of range.
bool load_row(const fx_kv_batch& in, size_t plane, uint32_t s, uint32_t k, Row& r) {
  r.a = FX_ORDER_REC(in.order[fx_index(k, s, in.steps)]);
  if (r.a >= in.steps) return false;
  const size_t at = fx_index(r.a, s, in.steps);
  r.key = in.key[at] & in.key_mask;
  for (uint32_t j = 0; j < FX_KV_MAX_OPS; ++j) r.op[j] = j < in.omax ? in.ops[j * plane + at] : FX_KV_OP(FX_KV_EMPTY, 0u);
  return r.key < in.keys;
}

// Order row k of a valid stream executed on the store `val`: its result words
// stored, what it leaves written to its key.  True: a write partial.
bool exec_row(const fx_kv_batch& in, size_t plane, uint32_t* result, uint32_t s, uint32_t k, uint32_t* val, Row& r) {
  load_row(in, plane, s, k, r);
  const fx::KvFold f = fx::kv_fold(r.op, in.omax);
  uint32_t res[FX_KV_MAX_OPS];
  fx::kv_walk(r.op, in.omax, val[r.key], res);
  const size_t at = fx_index(r.a, s, in.steps);
  for (uint32_t j = 0; j < in.omax; ++j) result[j * plane + at] = res[j];
  if (f.writes) val[r.key] = f.leaves;
  return f.writes;
}

uint32_t stream_status(const fx_kv_batch& in, size_t plane, uint32_t s) {
  const uint32_t ne = in.nexec[s];
  if (ne > in.steps) return FX_ERR_ORDER_OVERFLOW;
  Row r;
  for (uint32_t k = 0; k < ne; ++k)
    if (!load_row(in, plane, s, k, r) || fx::kv_fold(r.op, in.omax).bad) return FX_ERR_INVALID_ARG;
  return FX_OK;
}

// mon_off row of stream s ascending from 0 to at most steps, and every
// monitor row in use an arrival row below steps
bool monitor_ok(const fx_kv_monitor& m, uint32_t s) {
  if (s >= m.num_streams) return false;
  const uint32_t* off = m.mon_off + (size_t)s * (m.keys + 1u);
  if (off[0] != 0) return false;
  for (uint32_t k = 0; k < m.keys; ++k)
    if (off[k] > off[k + 1]) return false;
  if (off[m.keys] > m.steps) return false;
  for (uint32_t r = 0; r < off[m.keys]; ++r)
    if (m.monitor[fx_index(r, s, m.steps)] >= m.steps) return false;
  return true;
}

uint32_t rifl_at(const fx_kv_monitor& m, uint32_t s, uint32_t r) {
  return m.rifl[fx_index(m.monitor[fx_index(r, s, m.steps)], s, m.steps)];
}

}  // namespace

extern "C" {

int fx_kv_execute_host(const fx_kv_batch* inp, const fx_kv_out* out) {
  const int st = fx::kv_check(inp, out);
  if (st) return st;
  const fx_kv_batch& in = *inp;
  const size_t plane = fx_plane_words(in.num_streams, in.steps);
  const uint32_t keys = in.keys;
  for (uint32_t s = 0; s < in.num_streams; ++s) {
    const uint32_t status = stream_status(in, plane, s);
    out->err[s] = status;
    if (status) continue;
    const uint32_t ne = in.nexec[s];
    uint32_t* val = out->store + (size_t)s * keys;
    uint32_t* off = out->mon_off + (size_t)s * (keys + 1u);
    std::fill(val, val + keys, 0u);
    std::fill(off, off + keys + 1u, 0u);
    Row r;
    for (uint32_t k = 0; k < ne; ++k) {
      load_row(in, plane, s, k, r);
      if (fx::kv_fold(r.op, in.omax).writes) ++off[r.key + 1u];
    }
    for (uint32_t k = 0; k < keys; ++k) off[k + 1u] += off[k];
    std::vector<uint32_t> cursor(off, off + keys);
    for (uint32_t k = 0; k < ne; ++k)
      if (exec_row(in, plane, out->result, s, k, val, r)) out->monitor[fx_index(cursor[r.key]++, s, in.steps)] = r.a;
  }
  return FX_OK;
}

size_t fx_kv_session_bytes(uint32_t keys, uint32_t num_streams) {
  return (size_t)num_streams * fx::kv_session_stride(keys) * 4u;
}

// The sequential store over the session's state (fx_kv.h): the same header
// and table words as the device's after the same sequence of calls.
int fx_kv_advance_host(const fx_kv_batch* inp, const fx_kv_session_out* out, void* state, uint32_t flags) {
  const int st = fx::kv_advance_check(inp, out, state, flags);
  if (st) return st;
  const fx_kv_batch& in = *inp;
  const size_t plane = fx_plane_words(in.num_streams, in.steps);
  const uint32_t keys = in.keys, steps = in.steps;
  const bool init = (flags & FX_FLAG_INIT) != 0u;
  for (uint32_t s = 0; s < in.num_streams; ++s) {
    uint32_t* const H = (uint32_t*)state + (size_t)s * fx::kv_session_stride(keys);
    uint32_t* const val = H + fx::KV_H_WORDS;
    uint32_t* const cnt = val + fx::kv_session_keys(keys);
    const uint32_t ne = in.nexec[s];
    uint32_t done = 0;
    if (init) {
      std::fill(val, val + keys, 0u);
      std::fill(cnt, cnt + keys, 0u);
      if (ne > steps) {
        fx::kv_write_header(H, steps, keys, in.omax, 0u, FX_OK);
        out->err[s] = FX_ERR_ORDER_OVERFLOW;
        continue;
      }
    } else {
      done = H[fx::KV_H_DONE];
      const uint32_t status = H[fx::KV_H_ERR];
      if (!fx::kv_header_ok(H[fx::KV_H_TAG], H[fx::KV_H_STEPS], H[fx::KV_H_KEYS], H[fx::KV_H_OMAX], done, steps, keys,
                            in.omax)) {
        out->err[s] = FX_ERR_INVALID_ARG;
        continue;
      }
      if (status || ne > steps || ne <= done) {
        out->err[s] = status ? status : ne > steps ? FX_ERR_ORDER_OVERFLOW : ne < done ? FX_ERR_INVALID_ARG : FX_OK;
        continue;
      }
    }
    Row r;
    bool bad = false;
    for (uint32_t k = done; k < ne && !bad; ++k) bad = !load_row(in, plane, s, k, r) || fx::kv_fold(r.op, in.omax).bad;
    if (bad) {
      if (init) fx::kv_write_header(H, steps, keys, in.omax, 0u, FX_ERR_INVALID_ARG);
      H[fx::KV_H_ERR] = FX_ERR_INVALID_ARG;
      out->err[s] = FX_ERR_INVALID_ARG;
      continue;
    }
    for (uint32_t k = done; k < ne; ++k)
      if (exec_row(in, plane, out->result, s, k, val, r)) out->rank[fx_index(r.a, s, steps)] = cnt[r.key]++;
    std::copy(val, val + keys, out->store + (size_t)s * keys);
    fx::kv_write_header(H, steps, keys, in.omax, ne, FX_OK);
    out->err[s] = FX_OK;
  }
  return FX_OK;
}

int fx_kv_session_monitor_host(const fx_kv_batch* inp, const uint32_t* rank, const fx_kv_out* out, const void* state) {
  const int st = fx::kv_session_monitor_check(inp, rank, out, state);
  if (st) return st;
  const fx_kv_batch& in = *inp;
  const size_t plane = fx_plane_words(in.num_streams, in.steps);
  const uint32_t keys = in.keys, steps = in.steps;
  for (uint32_t s = 0; s < in.num_streams; ++s) {
    const uint32_t* const H = (const uint32_t*)state + (size_t)s * fx::kv_session_stride(keys);
    const uint32_t* const val = H + fx::KV_H_WORDS;
    const uint32_t* const cnt = val + fx::kv_session_keys(keys);
    const uint32_t done = H[fx::KV_H_DONE];
    if (!fx::kv_header_ok(H[fx::KV_H_TAG], H[fx::KV_H_STEPS], H[fx::KV_H_KEYS], H[fx::KV_H_OMAX], done, steps, keys,
                          in.omax)) {
      out->err[s] = FX_ERR_INVALID_ARG;
      continue;
    }
    uint32_t* off = out->mon_off + (size_t)s * (keys + 1u);
    uint64_t sum = 0;  // held at `steps`, as on the device
    for (uint32_t k = 0; k < keys; ++k) {
      off[k] = (uint32_t)sum;
      sum = std::min<uint64_t>(sum + cnt[k], steps);
    }
    off[keys] = (uint32_t)sum;
    std::copy(val, val + keys, out->store + (size_t)s * keys);
    Row r;
    for (uint32_t k = 0; k < done; ++k) {
      if (!load_row(in, plane, s, k, r) || !fx::kv_fold(r.op, in.omax).writes) continue;
      const uint32_t rk = rank[fx_index(r.a, s, steps)];
      if (rk < cnt[r.key] && (uint32_t)(off[r.key] + rk) < steps) out->monitor[fx_index(off[r.key] + rk, s, steps)] = r.a;
    }
    out->err[s] = H[fx::KV_H_ERR];
  }
  return FX_OK;
}

int fx_kv_monitor_compare_host(const fx_kv_monitor* a, const fx_kv_monitor* b, const uint32_t* pairs,
                               uint32_t num_pairs, uint32_t* diff) {
  const int st = fx::kv_monitor_check(a, b, pairs, num_pairs, diff);
  if (st) return st;
  for (uint32_t p = 0; p < num_pairs; ++p) {
    const uint32_t sa = pairs[2 * p], sb = pairs[2 * p + 1];
    uint32_t dk = FX_KV_AGREE, dp = FX_KV_AGREE;
    if (!monitor_ok(*a, sa) || !monitor_ok(*b, sb)) {
      dk = dp = FX_KV_BAD_PAIR;
    } else {
      const uint32_t* oa = a->mon_off + (size_t)sa * (a->keys + 1u);
      const uint32_t* ob = b->mon_off + (size_t)sb * (b->keys + 1u);
      for (uint32_t k = 0; k < a->keys && dk == FX_KV_AGREE; ++k) {
        const uint32_t la = oa[k + 1] - oa[k], lb = ob[k + 1] - ob[k], lo = std::min(la, lb);
        uint32_t i = 0;
        while (i < lo && rifl_at(*a, sa, oa[k] + i) == rifl_at(*b, sb, ob[k] + i)) ++i;
        if (i < lo || la != lb) dk = k, dp = i;
      }
    }
    diff[2 * p] = dk;
    diff[2 * p + 1] = dp;
  }
  return FX_OK;
}

int fx_kv_synth_ops_host(uint64_t seed, uint32_t stream_base, uint32_t read_pct, uint32_t delete_pct,
                         const uint32_t* lengths, uint32_t num_streams, uint32_t steps, uint32_t* ops) {
  const int st = fx::kv_synth_check(stream_base, read_pct, delete_pct, num_streams, ops);
  if (st) return st;
  const size_t plane = fx_plane_words(num_streams, steps);
  for (size_t w = 0; w < plane; ++w)
    ops[w] = fx::kv_synth_word(w, seed, stream_base, read_pct, delete_pct, lengths, num_streams, steps);
  return FX_OK;
}

}  // extern "C"
