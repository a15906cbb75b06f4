// kv_step.inc -- what a wavefront of the KV stage does with a chunk of 64 order
// rows, lane i holding one row: the one statement of it, included into the
// anonymous namespace of kv_exec.hip (k_kv_exec) and of kv_advance.hip
// (k_kv_advance, k_kv_session_monitor) behind fx_kv.h and fx_wave.h.
//
// A stream has two tables, the value of every key and a count of every key
// (k_kv_exec: the monitor cursor, k_kv_advance: the write partials executed so
// far), in LDS or in memory: the caller forms the two pointers.  Entry k of a
// table is read and written by lane k & 63 only, so a lane only ever reads back
// its own stores, in program order, and what the lanes of a chunk tell each
// other goes through registers (ballot, readlane, bpermute): no barrier, no
// atomic, every store a plain vector store.
//
//   kv_chunk_keys   for every distinct key k of the chunk (k = the key of the
//                   first unserved lane): m = ballot(key == k), w = m &
//                   ballot(writes); a lane of m finds the value left by the
//                   highest lane of w below it, else the table's; the owner
//                   stores the value the last lane of w leaves and adds
//                   popcount(w) to the key's count; a writing lane's place is
//                   the count before the chunk + popcount(w below it): its
//                   monitor row (k_kv_exec) or its rank (k_kv_advance)
//   kv_store_results   every lane walks its slots with the value it found and
//                   stores its result words

struct KvRow {
  uint32_t a, key;
  uint32_t op[FX_KV_MAX_OPS];
  bool in;   // the lane holds a row
  bool bad;  // arrival row or key out of range (then key is 0 and the ops EMPTY)
};

// Order row k of stream s, if the lane has one (`have`).  (The batch by value
// here and below: behind a reference the compiler no longer reads it as the
// kernel's arguments.)
__device__ __forceinline__ KvRow load_row(const fx_kv_batch in, size_t plane, uint32_t s, uint32_t k, bool have) {
  KvRow r;
  r.in = have;
  r.bad = false;
  r.a = 0;
  r.key = 0;
#pragma unroll
  for (uint32_t j = 0; j < FX_KV_MAX_OPS; ++j) r.op[j] = FX_KV_OP(FX_KV_EMPTY, 0u);
  if (r.in) {
    r.a = FX_ORDER_REC(in.order[fx_index(k, s, in.steps)]);
    if (r.a >= in.steps) {
      r.bad = true;
    } else {
      const size_t at = fx_index(r.a, s, in.steps);
      r.key = in.key[at] & in.key_mask;
#pragma unroll
      for (uint32_t j = 0; j < FX_KV_MAX_OPS; ++j)
        if (j < in.omax) r.op[j] = in.ops[j * plane + at];
      if (r.key >= in.keys) {
        r.bad = true;
        r.key = 0;
      }
    }
  }
  return r;
}

struct KvPlace {
  uint32_t found;  // the value the lane's partial found on its key
  uint32_t at;     // a writing lane: the key's count before it
};

// The distinct-key loop of a chunk whose rows are valid (every key < keys).
__device__ __forceinline__ KvPlace kv_chunk_keys(const KvRow& r, const fx::KvFold& f, bool wr, uint32_t* val,
                                                 uint32_t* cnt, uint32_t lane, uint64_t below) {
  const uint64_t writers = __ballot(wr);
  KvPlace p{0u, 0u};
  uint64_t un = __ballot(r.in);
  while (un) {
    const uint32_t k = fx::rl(r.key, (uint32_t)__builtin_ctzll(un));
    const uint32_t owner = k & 63u;
    const bool mine = r.in && r.key == k;
    const uint64_t m = __ballot(mine), w = m & writers;
    uint32_t tv = 0u, tc = 0u;
    if (lane == owner) {
      tv = val[k];
      tc = cnt[k];
    }
    tv = fx::rl(tv, owner);
    tc = fx::rl(tc, owner);
    const uint64_t wb = w & below;
    // the nearest writer of this key below the lane (every lane takes part in the exchange)
    const uint32_t src = wb ? 63u - (uint32_t)__builtin_clzll(wb) : lane;
    const uint32_t left = (uint32_t)__shfl((int)f.leaves, (int)src);
    if (mine) {
      p.found = wb ? left : tv;
      p.at = tc + (uint32_t)__builtin_popcountll(wb);
    }
    if (w) {
      const uint32_t last = fx::rl(f.leaves, 63u - (uint32_t)__builtin_clzll(w));
      if (lane == owner) {
        val[k] = last;
        cnt[k] = tc + (uint32_t)__builtin_popcountll(w);
      }
    }
    un &= ~m;
  }
  return p;
}

// The result words of the lane's row; returns the index of its arrival row.
__device__ __forceinline__ size_t kv_store_results(const fx_kv_batch in, size_t plane, uint32_t* result, uint32_t s,
                                                   const KvRow& r, uint32_t found) {
  uint32_t res[FX_KV_MAX_OPS];
  fx::kv_walk(r.op, in.omax, found, res);
  const size_t at = fx_index(r.a, s, in.steps);
#pragma unroll
  for (uint32_t j = 0; j < FX_KV_MAX_OPS; ++j)
    if (j < in.omax) result[j * plane + at] = res[j];
  return at;
}

struct KvHeader {
  bool ok;  // fx::kv_header_ok: a header a call with these steps, keys and omax may continue from
  uint32_t done, status;
};

// A session's header: lane 0 reads it, every lane gets it.
__device__ __forceinline__ KvHeader kv_read_header(const uint32_t* H, uint32_t lane, uint32_t steps, uint32_t keys,
                                                   uint32_t omax) {
  uint32_t tag = 0u, hsteps = 0u, hkeys = 0u, homax = 0u, done = 0u, status = 0u;
  if (lane == 0) {
    tag = H[fx::KV_H_TAG], hsteps = H[fx::KV_H_STEPS], hkeys = H[fx::KV_H_KEYS], homax = H[fx::KV_H_OMAX];
    done = H[fx::KV_H_DONE], status = H[fx::KV_H_ERR];
  }
  tag = fx::rl(tag, 0), hsteps = fx::rl(hsteps, 0), hkeys = fx::rl(hkeys, 0), homax = fx::rl(homax, 0);
  done = fx::rl(done, 0), status = fx::rl(status, 0);
  return KvHeader{fx::kv_header_ok(tag, hsteps, hkeys, homax, done, steps, keys, omax), done, status};
}
