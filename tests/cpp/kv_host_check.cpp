// The host twins of the KV stage (fx_kv_execute_host,
// fx_kv_monitor_compare_host, fx_kv_synth_ops_host) on buffers allocated at
// exactly the sizes the header states (planes of fx_plane_words words, store
// of S * keys, mon_off of S * (keys + 1)).  Built with
// -fsanitize=address,undefined (`make kv-check`), so a store one word outside
// a buffer, or a read of one, stops the program.  The outputs are also checked
// against a std::map store and per-key lists, and the words a call must leave
// alone against their sentinel.  Host only: no device.
#include <stdio.h>

#include <algorithm>
#include <map>
#include <random>
#include <vector>

#include "fantoch_amd.h"

namespace {

int failures = 0;
constexpr uint32_t A5 = 0xA5A5A5A5u;

#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      ++failures;                         \
      printf("FAILED %s: ", #cond);       \
      printf(__VA_ARGS__);                \
      printf("\n");                       \
    }                                     \
  } while (0)

struct Batch {
  uint32_t S, steps, keys, omax;
  std::vector<uint32_t> order, nexec, key, ops, rifl, result, store, monitor, mon_off, err;
  fx_kv_batch in;
  fx_kv_out out;
  Batch(uint32_t S_, uint32_t steps_, uint32_t keys_, uint32_t omax_) : S(S_), steps(steps_), keys(keys_), omax(omax_) {
    const size_t pw = fx_plane_words(S, steps);
    order.assign(pw, A5);
    key.assign(pw, A5);
    rifl.assign(pw, A5);
    ops.assign(pw * omax, A5);
    nexec.assign(S, 0);
    result.assign(pw * omax, A5);
    monitor.assign(pw, A5);
    store.assign((size_t)S * keys, A5);
    mon_off.assign((size_t)S * (keys + 1), A5);
    err.assign(S, A5);
    in = fx_kv_batch{order.data(), nexec.data(), key.data(), 0x00FFFFFFu, ops.data(), S, steps, keys, omax};
    out = fx_kv_out{result.data(), store.data(), monitor.data(), mon_off.data(), err.data()};
  }
  fx_kv_monitor mon() const { return fx_kv_monitor{monitor.data(), mon_off.data(), rifl.data(), S, steps, keys}; }
};

// Random streams: stream s executes nexec of its rows in a random order.
void fill(Batch& b, std::mt19937& rng, const std::vector<uint32_t>& counts) {
  const size_t pw = fx_plane_words(b.S, b.steps);
  for (uint32_t s = 0; s < b.S; ++s) {
    std::vector<uint32_t> rows(b.steps);
    for (uint32_t a = 0; a < b.steps; ++a) {
      rows[a] = a;
      const size_t at = fx_index(a, s, b.steps);
      b.key[at] = (rng() % b.keys) | 0x81000000u;
      b.rifl[at] = 1000u * s + a;
      const uint32_t used = rng() % (b.omax + 1u);
      for (uint32_t j = 0; j < b.omax; ++j) {
        const uint32_t kind = rng() % 3u;
        b.ops[j * pw + at] = j >= used ? FX_KV_OP(FX_KV_EMPTY, 0u) : FX_KV_OP(kind, kind == FX_KV_PUT ? 1u + rng() % 5u : 0u);
      }
    }
    for (uint32_t a = b.steps; a > 1; --a) std::swap(rows[a - 1], rows[rng() % a]);
    b.nexec[s] = std::min(counts[s % counts.size()], b.steps);
    for (uint32_t k = 0; k < b.nexec[s]; ++k)
      b.order[fx_index(k, s, b.steps)] = rows[k] | (k % 3u == 0 ? FX_ORDER_SCC_START : 0u);
  }
}

void check_against_a_map(const Batch& b) {
  const size_t pw = fx_plane_words(b.S, b.steps);
  for (uint32_t s = 0; s < b.S; ++s) {
    EXPECT(b.err[s] == FX_OK, "stream %u: status %u", s, b.err[s]);
    if (b.err[s]) continue;
    std::map<uint32_t, uint32_t> store;
    std::map<uint32_t, std::vector<uint32_t>> monitor;
    for (uint32_t k = 0; k < b.nexec[s]; ++k) {
      const uint32_t a = FX_ORDER_REC(b.order[fx_index(k, s, b.steps)]);
      const size_t at = fx_index(a, s, b.steps);
      const uint32_t key = b.key[at] & 0x00FFFFFFu;
      bool writes = false;
      for (uint32_t j = 0; j < b.omax; ++j) {
        const uint32_t op = b.ops[j * pw + at], kind = FX_KV_OP_KIND(op);
        uint32_t want = 0;
        if (kind == FX_KV_GET || kind == FX_KV_DELETE) want = store.count(key) ? store[key] : 0u;
        if (kind == FX_KV_PUT) store[key] = FX_KV_OP_VALUE(op);
        if (kind == FX_KV_DELETE) store.erase(key);
        writes = writes || kind == FX_KV_PUT || kind == FX_KV_DELETE;
        EXPECT(b.result[j * pw + at] == want, "stream %u row %u slot %u: %u, want %u", s, a, j, b.result[j * pw + at], want);
      }
      if (writes) monitor[key].push_back(a);
    }
    const uint32_t* off = b.mon_off.data() + (size_t)s * (b.keys + 1u);
    EXPECT(off[0] == 0, "stream %u: mon_off[0]", s);
    for (uint32_t k = 0; k < b.keys; ++k) {
      EXPECT(b.store[(size_t)s * b.keys + k] == (store.count(k) ? store[k] : 0u), "stream %u key %u: store", s, k);
      const std::vector<uint32_t>& want = monitor[k];
      EXPECT(off[k + 1] - off[k] == want.size(), "stream %u key %u: %u monitor rows", s, k, off[k + 1] - off[k]);
      for (uint32_t i = 0; i < want.size() && off[k] + i < b.steps; ++i)
        EXPECT(b.monitor[fx_index(off[k] + i, s, b.steps)] == want[i], "stream %u key %u row %u", s, k, i);
    }
    for (uint32_t r = off[b.keys]; r < b.steps; ++r)
      EXPECT(b.monitor[fx_index(r, s, b.steps)] == A5, "stream %u: monitor row %u past the end written", s, r);
  }
}

void run(uint32_t S, uint32_t steps, uint32_t keys, uint32_t omax, uint32_t seed) {
  std::mt19937 rng(seed);
  Batch b(S, steps, keys, omax);
  fill(b, rng, {0, 1, 63, 64, 65, 129, steps});
  EXPECT(fx_kv_execute_host(&b.in, &b.out) == FX_OK, "execute");
  check_against_a_map(b);
  // every stream against itself, and against its neighbour
  std::vector<uint32_t> pairs, diff(4 * (size_t)S, A5);
  for (uint32_t s = 0; s < S; ++s) {
    pairs.insert(pairs.end(), {s, s, s, (s + 1u) % S});
  }
  const fx_kv_monitor m = b.mon();
  EXPECT(fx_kv_monitor_compare_host(&m, &m, pairs.data(), 2 * S, diff.data()) == FX_OK, "compare");
  for (uint32_t s = 0; s < S; ++s)
    EXPECT(diff[4 * s] == FX_KV_AGREE && diff[4 * s + 1] == FX_KV_AGREE, "stream %u differs from itself", s);
  // an errored stream keeps its sentinel rows and cannot be compared
  if (steps >= 2) {
    Batch e(S, steps, keys, omax);
    fill(e, rng, {steps});
    e.order[fx_index(steps - 1, 0, steps)] = steps;
    if (S > 1) e.nexec[1] = steps + 1;
    EXPECT(fx_kv_execute_host(&e.in, &e.out) == FX_OK, "execute with bad streams");
    EXPECT(e.err[0] == FX_ERR_INVALID_ARG, "status %u", e.err[0]);
    if (S > 1) EXPECT(e.err[1] == FX_ERR_ORDER_OVERFLOW, "status %u", e.err[1]);
    for (uint32_t s = 0; s < std::min(S, 2u); ++s) {
      bool clean = true;
      for (uint32_t k = 0; k <= keys; ++k) clean = clean && e.mon_off[(size_t)s * (keys + 1u) + k] == A5;
      for (uint32_t k = 0; k < keys; ++k) clean = clean && e.store[(size_t)s * keys + k] == A5;
      for (uint32_t r = 0; r < steps; ++r)
        clean = clean && e.monitor[fx_index(r, s, steps)] == A5 && e.result[fx_index(r, s, steps)] == A5;
      EXPECT(clean, "stream %u wrote beside its status", s);
    }
    const fx_kv_monitor me = e.mon();
    const uint32_t pr[2] = {0, 0};
    uint32_t df[2] = {0, 0};
    EXPECT(fx_kv_monitor_compare_host(&me, &me, pr, 1, df) == FX_OK && df[0] == FX_KV_BAD_PAIR, "bad pair");
  }
}

void synth(uint32_t S, uint32_t steps) {
  std::vector<uint32_t> ops(fx_plane_words(S, steps), A5), lengths(S);
  for (uint32_t s = 0; s < S; ++s) lengths[s] = (7u * s) % (steps + 1u);
  EXPECT(fx_kv_synth_ops_host(3, 0xFFFFFFFFu - S + 1u, 40, 10, lengths.data(), S, steps, ops.data()) == FX_OK, "synth");
  const uint32_t spad = (S + 63u) / 64u * 64u, rows = (steps + 3u) / 4u * 4u;
  for (uint32_t s = 0; s < spad; ++s)
    for (uint32_t r = 0; r < rows; ++r) {
      const uint32_t op = ops[fx_index(r, s, steps)], kind = FX_KV_OP_KIND(op);
      if (s < S && r < lengths[s])
        EXPECT(kind != FX_KV_EMPTY && (kind != FX_KV_PUT || FX_KV_OP_VALUE(op) != 0), "stream %u row %u: %#x", s, r, op);
      else
        EXPECT(op == FX_KV_OP(FX_KV_EMPTY, 0u), "stream %u row %u: %#x past the length", s, r, op);
    }
}

}  // namespace

int main() {
  // (S, steps, keys, omax, seed)
  run(1, 1, 1, 1, 1);
  run(1, 131, 3, 4, 2);
  run(64, 66, 5, 2, 3);
  run(65, 130, 700, 1, 4);
  run(3, 7, 64, 3, 5);
  synth(1, 1);
  synth(65, 9);
  synth(130, 64);
  {
    Batch b(2, 8, 4, 2);
    fx_kv_batch in = b.in;
    in.omax = 5;
    EXPECT(fx_kv_execute_host(&in, &b.out) == FX_ERR_INVALID_ARG, "omax 5 accepted");
    in = b.in;
    in.keys = 0;
    EXPECT(fx_kv_execute_host(&in, &b.out) == FX_ERR_INVALID_ARG, "keys 0 accepted");
    EXPECT(b.err[0] == A5 && b.mon_off[0] == A5 && b.store[0] == A5, "a refused call wrote");
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("kv_host_check: ok\n");
  return 0;
}
