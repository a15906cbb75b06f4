// kv_exec.hip — KVStore results, final stores and per-key execution monitors of
// a batch (fx_kv_execute), the comparison of monitors (fx_kv_monitor_compare)
// and the op generator (fx_kv_synth_ops); the semantics of one partial and the
// draws: fx_kv.h; the host twins: kv_host.cpp.
//
// k_kv_exec: one wavefront per stream, 64 order rows per iteration, lane i
// holding row k0 + i: its arrival row, its key and its op words.  A stream has
// two tables, the value and the monitor cursor of every key: in LDS up to
// FX_KV_ONCHIP_KEYS keys, above in the stream's own store / mon_off rows (the
// cursor of key k in mon_off[k + 1], which it leaves holding the end of key k's
// monitor rows, i.e. the offset of key k + 1).  The row load, the owner-lane
// rule of the tables and the execute step of a chunk are stated once, in
// kv_step.inc, for this kernel and the sessions' (kv_advance.hip).
//
//   validate   arrival row < steps, key < keys, the op slots well formed; any
//              failure ends the stream with its status before it stored a word
//              (the HBM tier, whose tables are the caller's output rows, has a
//              pass of its own for this; the LDS tier does it while counting)
//   count      per chunk, for every distinct key k among the writing lanes
//              (k = the key of the first unserved lane): the owner adds
//              popcount(ballot(key == k)) to cursor[k]; then an exclusive
//              prefix over the keys, 64 at a time, makes the counts first rows
//   execute    per chunk kv_chunk_keys with the cursor as the key's count: a
//              writing lane's place is its monitor row; then kv_store_results
//              and the monitor row's store
#include <hip/hip_runtime.h>

#include "fx_kv.h"
#include "fx_wave.h"

namespace {

using fx::rl;

struct KvArgs {
  fx_kv_batch in;
  fx_kv_out out;
  size_t plane;
};

#include "kv_step.inc"

// (fx::wave_min's DPP steps would change k_kv_compare's code: this one stays)
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
    v = o < v ? o : v;
  }
  return v;
}

template <bool LDS>
__global__ __launch_bounds__(64) void k_kv_exec(const KvArgs a) {
  extern __shared__ uint32_t lds_tab[];  // LDS: value[keys], cursor[keys]
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  const uint32_t keys = a.in.keys, steps = a.in.steps, omax = a.in.omax;
  const uint32_t ne = a.in.nexec[s];
  if (ne > steps) {
    if (lane == 0) a.out.err[s] = FX_ERR_ORDER_OVERFLOW;
    return;
  }
  uint32_t* const off = a.out.mon_off + (size_t)s * (keys + 1u);
  uint32_t* const val = LDS ? lds_tab : a.out.store + (size_t)s * keys;
  uint32_t* const cur = LDS ? lds_tab + keys : off + 1;

  if (!LDS) {  // the tables are output rows: nothing may be stored before the stream is known to be valid
    bool bad = false;
    for (uint32_t k0 = 0; k0 < ne; k0 += 64u) {
      const KvRow r = load_row(a.in, a.plane, s, k0 + lane, k0 + lane < ne);
      bad |= r.bad || fx::kv_fold(r.op, omax).bad;
    }
    if (__ballot(bad)) {
      if (lane == 0) a.out.err[s] = FX_ERR_INVALID_ARG;
      return;
    }
  }
  for (uint32_t k = lane; k < keys; k += 64u) {
    val[k] = 0u;
    cur[k] = 0u;
  }

  // count the write partials of every key
  bool bad = false;
  for (uint32_t k0 = 0; k0 < ne; k0 += 64u) {
    const KvRow r = load_row(a.in, a.plane, s, k0 + lane, k0 + lane < ne);
    const fx::KvFold f = fx::kv_fold(r.op, omax);
    bad |= r.bad || f.bad;
    const bool wr = f.writes && !r.bad;
    uint64_t un = __ballot(wr);
    while (un) {
      const uint32_t k = rl(r.key, (uint32_t)__builtin_ctzll(un));
      const uint64_t w = __ballot(wr && r.key == k);
      if (lane == (k & 63u)) cur[k] += (uint32_t)__builtin_popcountll(w);
      un &= ~w;
    }
  }
  if (LDS && __ballot(bad)) {
    if (lane == 0) a.out.err[s] = FX_ERR_INVALID_ARG;
    return;
  }

  // counts -> first rows: lane l scans keys base + l (its own entries)
  uint32_t carry = 0;
  for (uint32_t base = 0; base < keys; base += 64u) {
    const uint32_t k = base + lane;
    const uint32_t c = k < keys ? cur[k] : 0u;
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= (uint32_t)d) incl += o;
    }
    if (k < keys) cur[k] = carry + incl - c;
    carry += rl(incl, 63u);
  }

  // execute
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t k0 = 0; k0 < ne; k0 += 64u) {
    const KvRow r = load_row(a.in, a.plane, s, k0 + lane, k0 + lane < ne);
    const fx::KvFold f = fx::kv_fold(r.op, omax);
    const bool wr = r.in && f.writes;
    const KvPlace p = kv_chunk_keys(r, f, wr, val, cur, lane, below);
    if (r.in) {
      kv_store_results(a.in, a.plane, a.out.result, s, r, p.found);
      if (wr) a.out.monitor[fx_index(p.at, s, steps)] = r.a;
    }
  }

  if (LDS)
    for (uint32_t k = lane; k < keys; k += 64u) {
      a.out.store[(size_t)s * keys + k] = val[k];
      off[k + 1u] = cur[k];
    }
  if (lane == 0) {
    off[0] = 0u;
    a.out.err[s] = FX_OK;
  }
}

struct CmpArgs {
  fx_kv_monitor a, b;
  const uint32_t* pairs;
  uint32_t* diff;
};

__device__ __forceinline__ uint32_t rifl_at(const fx_kv_monitor& m, uint32_t s, uint32_t r) {
  return m.rifl[fx_index(m.monitor[fx_index(r, s, m.steps)], s, m.steps)];
}

// One wavefront per pair.  The keys' lengths first: up to the first key kl
// whose lengths differ the two streams' rows of a key are the same linear
// rows, so the lanes compare linear rows up to the shorter end of key kl.
__global__ __launch_bounds__(64) void k_kv_compare(const CmpArgs c) {
  const uint32_t p = blockIdx.x, lane = threadIdx.x, keys = c.a.keys;
  const uint32_t sa = c.pairs[2u * p], sb = c.pairs[2u * p + 1u];
  uint32_t dk = FX_KV_AGREE, dp = FX_KV_AGREE;
  bool ok = sa < c.a.num_streams && sb < c.b.num_streams;
  const uint32_t* oa = c.a.mon_off + (size_t)(ok ? sa : 0u) * (keys + 1u);
  const uint32_t* ob = c.b.mon_off + (size_t)(ok ? sb : 0u) * (keys + 1u);
  if (ok) {
    bool bad = oa[0] != 0u || ob[0] != 0u || oa[keys] > c.a.steps || ob[keys] > c.b.steps;
    for (uint32_t k = lane; k < keys; k += 64u) bad |= oa[k] > oa[k + 1u] || ob[k] > ob[k + 1u];
    ok = !__ballot(bad);
  }
  if (ok) {
    bool bad = false;
    for (uint32_t r = lane; r < oa[keys]; r += 64u) bad |= c.a.monitor[fx_index(r, sa, c.a.steps)] >= c.a.steps;
    for (uint32_t r = lane; r < ob[keys]; r += 64u) bad |= c.b.monitor[fx_index(r, sb, c.b.steps)] >= c.b.steps;
    ok = !__ballot(bad);
  }
  if (!ok) {
    dk = dp = FX_KV_BAD_PAIR;
  } else {
    uint32_t kl = FX_KV_AGREE;
    for (uint32_t k = lane; k < keys && kl == FX_KV_AGREE; k += 64u)
      if (oa[k + 1u] - oa[k] != ob[k + 1u] - ob[k]) kl = k;
    kl = wave_min(kl);
    uint32_t limit = oa[keys], shorter = 0u;
    if (kl != FX_KV_AGREE) {
      const uint32_t la = oa[kl + 1u] - oa[kl], lb = ob[kl + 1u] - ob[kl];
      shorter = la < lb ? la : lb;
      limit = oa[kl] + shorter;
    }
    uint32_t at = FX_KV_AGREE;
    for (uint32_t r0 = 0; r0 < limit; r0 += 64u) {
      const uint32_t r = r0 + lane;
      const uint64_t d = __ballot(r < limit && rifl_at(c.a, sa, r) != rifl_at(c.b, sb, r));
      if (d) {
        at = r0 + (uint32_t)__builtin_ctzll(d);
        break;
      }
    }
    if (at != FX_KV_AGREE) {  // the key whose rows hold linear row `at`: oa[lo] <= at < oa[lo + 1]
      uint32_t lo = 0, hi = keys;
      while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (oa[mid] <= at) lo = mid; else hi = mid;
      }
      dk = lo;
      dp = at - oa[lo];
    } else if (kl != FX_KV_AGREE) {
      dk = kl;
      dp = shorter;
    }
  }
  if (lane == 0) {
    c.diff[2u * p] = dk;
    c.diff[2u * p + 1u] = dp;
  }
}

__global__ __launch_bounds__(256) void k_kv_synth_ops(uint64_t seed, uint32_t stream_base, uint32_t read_pct,
                                                      uint32_t delete_pct, const uint32_t* lengths, uint32_t S,
                                                      uint32_t steps, uint32_t* ops, size_t plane) {
  const size_t w = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (w < plane) ops[w] = fx::kv_synth_word(w, seed, stream_base, read_pct, delete_pct, lengths, S, steps);
}

}  // namespace

extern "C" int fx_kv_execute(const fx_kv_batch* in, const fx_kv_out* out, void* hip_stream) {
  const int st = fx::kv_check(in, out);
  if (st) return st;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (in->num_streams == 0) return FX_OK;
  if (in->num_streams > 0x7FFFFFFFu) return FX_ERR_INVALID_ARG;
  const KvArgs a{*in, *out, fx_plane_words(in->num_streams, in->steps)};
  hipStream_t hs = (hipStream_t)hip_stream;
  if (in->keys <= FX_KV_ONCHIP_KEYS)
    hipLaunchKernelGGL(k_kv_exec<true>, dim3(in->num_streams), dim3(64), (size_t)in->keys * 8u, hs, a);
  else
    hipLaunchKernelGGL(k_kv_exec<false>, dim3(in->num_streams), dim3(64), 0, hs, a);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}

extern "C" int fx_kv_monitor_compare(const fx_kv_monitor* a, const fx_kv_monitor* b, const uint32_t* pairs,
                                     uint32_t num_pairs, uint32_t* diff, void* hip_stream) {
  const int st = fx::kv_monitor_check(a, b, pairs, num_pairs, diff);
  if (st) return st;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (num_pairs == 0) return FX_OK;
  if (num_pairs > 0x7FFFFFFFu) return FX_ERR_INVALID_ARG;
  const CmpArgs c{*a, *b, pairs, diff};
  hipLaunchKernelGGL(k_kv_compare, dim3(num_pairs), dim3(64), 0, (hipStream_t)hip_stream, c);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}

extern "C" int fx_kv_synth_ops(uint64_t seed, uint32_t stream_base, uint32_t read_pct, uint32_t delete_pct,
                               const uint32_t* lengths, uint32_t num_streams, uint32_t steps, uint32_t* ops,
                               void* hip_stream) {
  const int st = fx::kv_synth_check(stream_base, read_pct, delete_pct, num_streams, ops);
  if (st) return st;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  const size_t plane = fx_plane_words(num_streams, steps);
  if (plane == 0) return FX_OK;
  if (plane / 256u > 0x7FFFFFFFu) return FX_ERR_INVALID_ARG;
  hipLaunchKernelGGL(k_kv_synth_ops, dim3((uint32_t)(plane / 256u)), dim3(256), 0, (hipStream_t)hip_stream, seed,
                     stream_base, read_pct, delete_pct, lengths, num_streams, steps, ops, plane);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}
