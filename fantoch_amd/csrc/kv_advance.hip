// kv_advance.hip — resumable streams of the KV stage (fx_kv_advance) and the
// monitor of the rows a session has consumed (fx_kv_session_monitor):
// k_kv_exec's execute step continued from a saved store.  That step, the row
// load and the header read are stated once, in kv_step.inc, for these kernels
// and for k_kv_exec (kv_exec.hip).  The semantics: fantoch_amd.h; the state
// layout, the argument checks, the header check and the header write, shared
// with the host twin (kv_host.cpp): fx_kv.h.
//
// k_kv_advance: a wavefront per stream and workgroup, 64 order rows per
// iteration, lane i holding row k0 + i, k0 = done, done + 64, ...  Per stream
// the state is a header {tag, steps, keys, omax, done, err} and two tables,
// the value of every key and the write partials executed on it so far.  Up to
// FX_KV_ONCHIP_KEYS keys a call stages both in LDS (a load and a store of 8 B
// x keys per call) and works there; above, it works in the state itself.
//   header    lane 0 reads it before anything of the launch is stored; it is
//             validated (fx::kv_header_ok) before anything of it is used
//   validate  the call's own rows, [done, nexec): arrival row < steps, key <
//             keys, the op slots well formed.  A failure stops the stream: the
//             header's err alone is written, nothing of the call is stored
//   execute   per chunk kv_chunk_keys with the key's count: a writing lane's
//             place is its rank; then kv_store_results and the rank's store
//   store     every key's value, by its owner lane; the header, by lane 0, last
// With FX_FLAG_INIT the tables are cleared first (in the state, so that a call
// that stops at once leaves an empty store behind) and nothing of the state is
// read.
//
// k_kv_session_monitor: a wavefront per stream.  mon_off = the exclusive
// prefix of the counts, lane l scanning its own entries base + l, 64 at a
// time.  Then the consumed rows again, [0, done): for every distinct key of a
// chunk's writing lanes the owner lane reads mon_off[k] back (its own store),
// the lanes of the key get it through readlane, and monitor[mon_off[k] +
// rank[a]] = a.  A rank at or above the key's count (a rank plane that is not
// the session's) is skipped: no row outside the key's own rows is written.
//
// There is no barrier, no spin loop and no atomic; every store is a plain
// vector store; lanes tell each other things through ballot, readlane and
// shuffles only.  Every loop is bounded by nexec, done (<= steps, checked) or
// keys, and every index taken from memory is checked before it is used.
#include <hip/hip_runtime.h>

#include "fx_internal.h"
#include "fx_kv.h"
#include "fx_wave.h"

namespace {

using fx::rl;

struct KaArgs {
  fx_kv_batch in;
  fx_kv_session_out out;
  size_t plane;
  uint32_t* state;
  uint32_t init;
};

struct KmArgs {
  fx_kv_batch in;
  fx_kv_out out;
  size_t plane;
  const uint32_t* rank;
  const uint32_t* state;
};

#include "kv_step.inc"

template <bool LDS>
__global__ __launch_bounds__(64) void k_kv_advance(const KaArgs a) {
  extern __shared__ uint32_t lds_tab[];  // LDS: value[keys], count[keys]
  const uint32_t s = fx::xcd_slot(blockIdx.x), lane = threadIdx.x;
  if (s >= a.in.num_streams) return;
  const uint32_t keys = a.in.keys, steps = a.in.steps, omax = a.in.omax;
  const uint32_t ne = a.in.nexec[s];
  uint32_t* const H = a.state + (size_t)s * fx::kv_session_stride(keys);
  uint32_t* const sval = H + fx::KV_H_WORDS;
  uint32_t* const scnt = sval + fx::kv_session_keys(keys);
  uint32_t* const val = LDS ? lds_tab : sval;
  uint32_t* const cnt = LDS ? lds_tab + keys : scnt;
  uint32_t done = 0u;

  if (a.init) {
    for (uint32_t k = lane; k < keys; k += 64u) {
      sval[k] = 0u;
      scnt[k] = 0u;
    }
    if (ne > steps) {  // an empty session: a proper call behind this one starts at row 0
      if (lane == 0) {
        fx::kv_write_header(H, steps, keys, omax, 0u, FX_OK);
        a.out.err[s] = FX_ERR_ORDER_OVERFLOW;
      }
      return;
    }
  } else {
    const KvHeader h = kv_read_header(H, lane, steps, keys, omax);
    if (!h.ok) {
      if (lane == 0) a.out.err[s] = FX_ERR_INVALID_ARG;
      return;
    }
    done = h.done;
    const uint32_t status = h.status;
    // a stream that stopped stays stopped; one with no new rows is done
    if (status || ne > steps || ne <= done) {
      if (lane == 0)
        a.out.err[s] = status ? status : ne > steps ? FX_ERR_ORDER_OVERFLOW : ne < done ? FX_ERR_INVALID_ARG : FX_OK;
      return;
    }
  }

  // validate the call's own rows before anything of them is stored
  {
    bool bad = false;
    for (uint32_t k0 = done; k0 < ne; k0 += 64u) {
      const KvRow r = load_row(a.in, a.plane, s, k0 + lane, k0 + lane < ne);
      bad |= r.bad || fx::kv_fold(r.op, omax).bad;
    }
    if (__ballot(bad)) {
      if (lane == 0) {
        if (a.init) fx::kv_write_header(H, steps, keys, omax, 0u, FX_ERR_INVALID_ARG);
        H[fx::KV_H_ERR] = FX_ERR_INVALID_ARG;
        a.out.err[s] = FX_ERR_INVALID_ARG;
      }
      return;
    }
  }

  if (LDS)
    for (uint32_t k = lane; k < keys; k += 64u) {
      val[k] = a.init ? 0u : sval[k];
      cnt[k] = a.init ? 0u : scnt[k];
    }

  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t k0 = done; k0 < ne; k0 += 64u) {
    const KvRow r = load_row(a.in, a.plane, s, k0 + lane, k0 + lane < ne);
    const fx::KvFold f = fx::kv_fold(r.op, omax);
    const bool wr = r.in && f.writes;
    const KvPlace p = kv_chunk_keys(r, f, wr, val, cnt, lane, below);  // the rows are valid
    if (r.in) {
      const size_t at = kv_store_results(a.in, a.plane, a.out.result, s, r, p.found);
      if (wr) a.out.rank[at] = p.at;
    }
  }

  for (uint32_t k = lane; k < keys; k += 64u) {
    const uint32_t v = val[k];
    a.out.store[(size_t)s * keys + k] = v;
    if (LDS) {
      sval[k] = v;
      scnt[k] = cnt[k];
    }
  }
  if (lane == 0) {
    fx::kv_write_header(H, steps, keys, omax, ne, FX_OK);
    a.out.err[s] = FX_OK;
  }
}

__global__ __launch_bounds__(64) void k_kv_session_monitor(const KmArgs a) {
  const uint32_t s = fx::xcd_slot(blockIdx.x), lane = threadIdx.x;
  if (s >= a.in.num_streams) return;
  const uint32_t keys = a.in.keys, steps = a.in.steps, omax = a.in.omax;
  const uint32_t* const H = a.state + (size_t)s * fx::kv_session_stride(keys);
  const uint32_t* const sval = H + fx::KV_H_WORDS;
  const uint32_t* const scnt = sval + fx::kv_session_keys(keys);
  const KvHeader h = kv_read_header(H, lane, steps, keys, omax);
  if (!h.ok) {
    if (lane == 0) a.out.err[s] = FX_ERR_INVALID_ARG;
    return;
  }
  const uint32_t done = h.done, status = h.status;
  uint32_t* const off = a.out.mon_off + (size_t)s * (keys + 1u);

  // counts -> first rows: lane l scans keys base + l (its own entries); a sum
  // that passes `steps` (counts that are not a session's) is held there
  uint32_t carry = 0;
  for (uint32_t base = 0; base < keys; base += 64u) {
    const uint32_t k = base + lane;
    uint32_t c = k < keys ? scnt[k] : 0u;
    c = c < steps ? c : steps;
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= (uint32_t)d) incl += o;
      incl = incl < steps ? incl : steps;
    }
    uint32_t first = carry + incl - c;
    first = first < steps ? first : steps;
    if (k < keys) {
      off[k] = first;
      a.out.store[(size_t)s * keys + k] = sval[k];
    }
    carry += rl(incl, 63u);
    carry = carry < steps ? carry : steps;
  }

  for (uint32_t k0 = 0; k0 < done; k0 += 64u) {
    const KvRow r = load_row(a.in, a.plane, s, k0 + lane, k0 + lane < done);
    const bool wr = r.in && !r.bad && fx::kv_fold(r.op, omax).writes;
    uint32_t first = 0u, count = 0u;
    uint64_t un = __ballot(wr);
    while (un) {
      const uint32_t k = rl(r.key, (uint32_t)__builtin_ctzll(un));  // < keys: load_row checked it
      const uint32_t owner = k & 63u;
      const uint64_t m = __ballot(wr && r.key == k);
      uint32_t tf = 0u, tc = 0u;
      if (lane == owner) {
        tf = off[k];
        tc = scnt[k];
      }
      tf = rl(tf, owner);
      tc = rl(tc, owner);
      if (wr && r.key == k) {
        first = tf;
        count = tc;
      }
      un &= ~m;
    }
    if (wr) {
      const uint32_t rk = a.rank[fx_index(r.a, s, steps)];
      if (rk < count && first + rk < steps) a.out.monitor[fx_index(first + rk, s, steps)] = r.a;
    }
  }
  if (lane == 0) {
    off[keys] = carry;
    a.out.err[s] = status;
  }
}

}  // namespace

using namespace fx;

extern "C" int fx_kv_advance(const fx_kv_batch* in, const fx_kv_session_out* out, void* state, uint32_t flags,
                             void* hip_stream) {
  const int st = kv_advance_check(in, out, state, flags);
  if (st) return st;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (in->num_streams == 0) return FX_OK;
  if (in->num_streams > 0x7FFFFFC0u) return FX_ERR_INVALID_ARG;
  const KaArgs a{*in, *out, fx_plane_words(in->num_streams, in->steps), (uint32_t*)state,
                 (flags & FX_FLAG_INIT) ? 1u : 0u};
  hipStream_t hs = (hipStream_t)hip_stream;
  const dim3 grid(xcd_grid(in->num_streams));
  if (in->keys <= FX_KV_ONCHIP_KEYS)
    hipLaunchKernelGGL(k_kv_advance<true>, grid, dim3(64), (size_t)in->keys * 8u, hs, a);
  else
    hipLaunchKernelGGL(k_kv_advance<false>, grid, dim3(64), 0, hs, a);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}

extern "C" int fx_kv_session_monitor(const fx_kv_batch* in, const uint32_t* rank, const fx_kv_out* out,
                                     const void* state, void* hip_stream) {
  const int st = kv_session_monitor_check(in, rank, out, state);
  if (st) return st;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  if (in->num_streams == 0) return FX_OK;
  if (in->num_streams > 0x7FFFFFC0u) return FX_ERR_INVALID_ARG;
  const KmArgs a{*in, *out, fx_plane_words(in->num_streams, in->steps), rank, (const uint32_t*)state};
  hipLaunchKernelGGL(k_kv_session_monitor, dim3(xcd_grid(in->num_streams)), dim3(64), 0, (hipStream_t)hip_stream, a);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}
