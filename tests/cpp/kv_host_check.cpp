// The host twins of the KV stage (fx_kv_execute_host,
// fx_kv_monitor_compare_host, fx_kv_synth_ops_host) on buffers allocated at
// exactly the sizes the header states (planes of fx_plane_words words, store
// of S * keys, mon_off of S * (keys + 1)).  Built with
// -fsanitize=address,undefined (`make kv-check`), so a store one word outside
// a buffer, or a read of one, stops the program.  The outputs are also checked
// against a std::map store and per-key lists, and the words a call must leave
// alone against their sentinel.  The comparison also runs over hand-built
// monitors of several key strips and row chunks, and over one pair per rule of
// a pair that cannot be compared.  Host only: no device.
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

// Hand-built monitors for fx_kv_monitor_compare_host: stream s holds len[k] commands on key k, command i of key
// k named 0x01000000 + (k << 12) + i, the command of monitor row r arriving at row (up ? r : steps - 1 - r).
struct Mon {
  uint32_t S, steps, keys;
  std::vector<uint32_t> monitor, mon_off, rifl;
  Mon(uint32_t S_, uint32_t steps_, uint32_t keys_) : S(S_), steps(steps_), keys(keys_) {
    monitor.assign(fx_plane_words(S, steps), A5);
    rifl.assign(fx_plane_words(S, steps), A5);
    mon_off.assign((size_t)S * (keys + 1), A5);
  }
  uint32_t& off(uint32_t s, uint32_t k) { return mon_off[(size_t)s * (keys + 1u) + k]; }
  uint32_t& row(uint32_t s, uint32_t r) { return monitor[fx_index(r, s, steps)]; }
  void set(uint32_t s, const std::vector<uint32_t>& len, bool up) {
    uint32_t r = 0;
    for (uint32_t k = 0; k < keys; ++k) {
      off(s, k) = r;
      for (uint32_t i = 0; i < len[k]; ++i, ++r) {
        const uint32_t a = up ? r : steps - 1u - r;
        row(s, r) = a;
        rifl[fx_index(a, s, steps)] = 0x01000000u + (k << 12) + i;
      }
    }
    off(s, keys) = r;
  }
  // another command on linear row r
  void alter(uint32_t s, uint32_t r) { rifl[fx_index(row(s, r), s, steps)] |= 0x40000000u; }
  fx_kv_monitor mon() const { return fx_kv_monitor{monitor.data(), mon_off.data(), rifl.data(), S, steps, keys}; }
};

void expect_diff(const Mon& a, const Mon& b, const std::vector<uint32_t>& pairs, const std::vector<uint32_t>& want,
                 const char* what) {
  const Mon before_a = a, before_b = b;
  std::vector<uint32_t> diff(pairs.size(), A5);  // exactly 2 words per pair
  const fx_kv_monitor ma = a.mon(), mb = b.mon();
  EXPECT(fx_kv_monitor_compare_host(&ma, &mb, pairs.data(), (uint32_t)pairs.size() / 2u, diff.data()) == FX_OK, "%s", what);
  for (size_t i = 0; i < want.size(); i += 2)
    EXPECT(diff[i] == want[i] && diff[i + 1] == want[i + 1], "%s: pair %zu (%u, %u): (%u, %u), want (%u, %u)", what, i / 2,
           pairs[i], pairs[i + 1], diff[i], diff[i + 1], want[i], want[i + 1]);
  EXPECT(a.monitor == before_a.monitor && a.mon_off == before_a.mon_off && a.rifl == before_a.rifl &&
             b.monitor == before_b.monitor && b.mon_off == before_b.mon_off && b.rifl == before_b.rifl,
         "%s: an input changed", what);
}

// 129 keys (three strips of 64) and 130 rows (three chunks of 64): side a fills every one of its rows.
void monitors_multi_strip() {
  const uint32_t keys = 129, AG = FX_KV_AGREE;
  std::vector<uint32_t> len(keys, 1u);
  len[0] = 2;  // key k > 0 holds linear row k + 1
  Mon a(1, 130, keys), b(5, 133, keys);
  a.set(0, len, true);
  std::vector<uint32_t> longer = len;
  longer[65] = 2;
  b.set(0, len, false);     // the same commands, arrived in the opposite order
  b.set(1, longer, false);  // a length difference at key 65
  b.set(2, longer, false);  // ... and a content difference at linear row 64, below it: key 63
  b.alter(2, 64);
  b.set(3, longer, false);  // ... and one at linear row 100, above it: not reported
  b.alter(3, 100);
  b.set(4, len, false);     // a content difference at linear row 64 alone
  b.alter(4, 64);
  EXPECT(a.off(0, keys) == a.steps, "side a is not full");
  const std::vector<uint32_t> pairs = {0, 0, 0, 1, 0, 2, 0, 3, 0, 4}, want = {AG, AG, 65, 1, 63, 0, 65, 1, 63, 0};
  expect_diff(a, b, pairs, want, "multi-strip");
  std::vector<uint32_t> back;
  for (size_t i = 0; i < pairs.size(); i += 2) back.insert(back.end(), {pairs[i + 1], pairs[i]});
  expect_diff(b, a, back, want, "multi-strip, sides swapped");
}

// One pair per rule of a stream that cannot be compared, on side a alone and on side b alone, between a pair
// that agrees and one that differs; every corruption keeps what a call may follow inside the buffers.
void monitors_bad_pairs() {
  const uint32_t keys = 129, steps = 131, AG = FX_KV_AGREE, BP = FX_KV_BAD_PAIR;
  std::vector<uint32_t> len(keys, 0u);
  for (uint32_t k = 0; k < keys; k += 2) len[k] = 1;
  len[5] = 3;  // 68 rows
  Mon bad(9, steps, keys), good(2, 140, keys);
  for (uint32_t s = 0; s < bad.S; ++s)
    if (s != 8) bad.set(s, len, true);  // stream 8: its mon_off row as an errored stream leaves it
  good.set(0, len, false);
  good.set(1, len, false);
  good.alter(1, 66);
  bad.off(1, 0) = 1;                              // does not start at 0
  bad.off(2, 65) = bad.off(2, 64) - 1u;           // decreases at key 64
  bad.off(3, keys) = bad.off(3, keys - 1u) - 1u;  // decreases at the last key
  bad.off(4, keys) = steps + 1u;                  // ends above steps
  bad.row(5, 0) = steps;                          // a monitor row in use that names no arrival row
  bad.row(6, 67) = 0x7FFFFFFFu;                   // the last row in use
  bad.row(7, 68) = steps;                         // the first row not in use: legal
  std::vector<uint32_t> pairs, want, back;
  for (uint32_t s : {1u, 2u, 3u, 4u, 5u, 6u, 8u, 9u, 0x80000005u}) {  // 9: num_streams; one far above
    pairs.insert(pairs.end(), {0, 0, s, 0, 0, 1});
    want.insert(want.end(), {AG, AG, BP, BP, 126, 0});  // linear row 66: key 5's three rows, the even keys below 126 one each
  }
  pairs.insert(pairs.end(), {7, 0, 7, 1});
  want.insert(want.end(), {AG, AG, 126, 0});
  for (size_t i = 0; i < pairs.size(); i += 2) back.insert(back.end(), {pairs[i + 1], pairs[i]});
  expect_diff(bad, good, pairs, want, "bad pairs on side a");
  expect_diff(good, bad, back, want, "bad pairs on side b");
  // every row in use and mon_off[keys] one above: the pad row `steps` of the plane names an arrival row, so
  // nothing but the offset itself tells
  static_assert(steps % 4u != 0, "steps needs a pad row");
  std::vector<uint32_t> all = len;
  all[7] = steps - 68;
  Mon full(1, steps, keys);
  full.set(0, all, true);
  EXPECT(full.off(0, keys) == steps, "the monitor is not full");
  expect_diff(full, good, {0, 0, 0, 1}, {7, 0, 7, 0}, "a full monitor");
  full.off(0, keys) = steps + 1u;
  full.row(0, steps) = 0;
  expect_diff(full, good, {0, 0}, {BP, BP}, "one row more than steps on side a");
  expect_diff(good, full, {0, 0}, {BP, BP}, "one row more than steps on side b");
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
  monitors_multi_strip();
  monitors_bad_pairs();
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
