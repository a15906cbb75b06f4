// The host twin of the pending stage (fx_pending_aggregate_host) on buffers
// allocated at exactly the sizes the header states (planes of fx_plane_words
// words, FX_PENDING_MAX_PARTS of them for `part`).  Built with
// -fsanitize=address,undefined (`make pending-check`), so a store one word
// outside a buffer, or a read of one, stops the program.  The outputs are also
// checked against a std::map of builders, and the words a call must leave alone
// against their sentinel.  Host only: no device.
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
  uint32_t S, steps;
  std::vector<uint32_t> order, nexec, rifl, count, part, head, ready, index, nready, nopen, err;
  fx_pending_batch in;
  fx_pending_out out;
  Batch(uint32_t S_, uint32_t steps_) : S(S_), steps(steps_) {
    const size_t pw = fx_plane_words(S, steps);
    order.assign(pw, A5);
    rifl.assign(pw, A5);
    count.assign(pw, A5);
    nexec.assign(S, 0);
    part.assign(pw * FX_PENDING_MAX_PARTS, A5);
    head.assign(pw, A5);
    ready.assign(pw, A5);
    index.assign(pw, A5);
    nready.assign(S, A5);
    nopen.assign(S, A5);
    err.assign(S, A5);
    in = fx_pending_batch{order.data(), nexec.data(), rifl.data(), count.data(), 0xFFu, 0u, S, steps};
    out = fx_pending_out{part.data(), head.data(), ready.data(), index.data(), nready.data(), nopen.data(), err.data()};
  }
};

// Random streams of 1- to 8-key commands whose partials are spread over the
// stream; stream s executes the first nexec rows of a random order.
void fill(Batch& b, std::mt19937& rng, const std::vector<uint32_t>& counts) {
  for (uint32_t s = 0; s < b.S; ++s) {
    std::vector<uint32_t> rows(b.steps);
    uint32_t a = 0, cmd = 0;
    while (a < b.steps) {
      const uint32_t c = std::min<uint32_t>(1u + rng() % (rng() % 4u ? 2u : 8u), b.steps - a);
      const bool ignored = rng() % 7u == 0;
      for (uint32_t j = 0; j < c; ++j, ++a) {
        const size_t at = fx_index(a, s, b.steps);
        b.rifl[at] = ((1u + cmd % 3u) << 24) | cmd;
        b.count[at] = FX_TABLE_PS_WORD(ignored ? 0u : c, 1u + rng() % 3u);
      }
      ++cmd;
    }
    for (uint32_t i = 0; i < b.steps; ++i) rows[i] = i;
    for (uint32_t i = b.steps; i > 1; --i) std::swap(rows[i - 1], rows[rng() % i]);
    b.nexec[s] = std::min(counts[s % counts.size()], b.steps);
    for (uint32_t k = 0; k < b.nexec[s]; ++k)
      b.order[fx_index(k, s, b.steps)] = rows[k] | (k % 3u == 0 ? FX_ORDER_SCC_START : 0u);
  }
}

struct Open {
  uint32_t head, count, got;
};

void check_against_a_map(const Batch& b, uint32_t process) {
  const size_t pw = fx_plane_words(b.S, b.steps);
  std::vector<bool> part_set(pw * FX_PENDING_MAX_PARTS), head_set(pw), index_set(pw), ready_set(pw);
  for (uint32_t s = 0; s < b.S; ++s) {
    EXPECT(b.err[s] == FX_OK, "stream %u: status %u", s, b.err[s]);
    if (b.err[s]) continue;
    std::map<uint32_t, Open> live;
    uint32_t nready = 0;
    for (uint32_t k = 0; k < b.nexec[s]; ++k) {
      const uint32_t a = FX_ORDER_REC(b.order[fx_index(k, s, b.steps)]);
      const size_t at = fx_index(a, s, b.steps);
      const uint32_t r = b.rifl[at];
      uint32_t c = FX_TABLE_PS_WORD_NKEYS(b.count[at]);
      if (process && (r >> 24) != process) c = 0;
      head_set[at] = true;
      if (c == 0) {
        EXPECT(b.head[at] == FX_PENDING_IGNORED, "stream %u row %u: head %u of an ignored row", s, a, b.head[at]);
        continue;
      }
      Open one{a, 1, 0};
      Open& o = c == 1 ? one : live.count(r) ? live[r] : (live[r] = Open{a, c, 0});
      const size_t hat = fx_index(o.head, s, b.steps);
      EXPECT(b.head[at] == o.head, "stream %u row %u: head %u, want %u", s, a, b.head[at], o.head);
      EXPECT(b.part[o.got * pw + hat] == a, "stream %u row %u: slot %u of head %u", s, a, o.got, o.head);
      part_set[o.got * pw + hat] = true;
      if (++o.got == c) {
        EXPECT(b.index[hat] == nready, "stream %u head %u: index %u, want %u", s, o.head, b.index[hat], nready);
        EXPECT(b.ready[fx_index(nready, s, b.steps)] == o.head, "stream %u: ready row %u", s, nready);
        index_set[hat] = ready_set[fx_index(nready, s, b.steps)] = true;
        ++nready;
        if (c > 1) live.erase(r);
      }
    }
    EXPECT(b.nready[s] == nready, "stream %u: nready %u, want %u", s, b.nready[s], nready);
    EXPECT(b.nopen[s] == live.size(), "stream %u: nopen %u, want %zu", s, b.nopen[s], live.size());
  }
  for (size_t w = 0; w < pw; ++w) {
    EXPECT(head_set[w] || b.head[w] == A5, "head word %zu written", w);
    EXPECT(index_set[w] || b.index[w] == A5, "index word %zu written", w);
    EXPECT(ready_set[w] || b.ready[w] == A5, "ready word %zu written", w);
  }
  for (size_t w = 0; w < pw * FX_PENDING_MAX_PARTS; ++w) EXPECT(part_set[w] || b.part[w] == A5, "part word %zu written", w);
}

void run(uint32_t S, uint32_t steps, uint32_t process, uint32_t seed) {
  std::mt19937 rng(seed);
  Batch b(S, steps);
  b.in.process = process;
  fill(b, rng, {0, 1, 63, 64, 65, 129, steps});
  EXPECT(fx_pending_aggregate_host(&b.in, &b.out, FX_PENDING_TIER_HBM) == FX_OK, "aggregate");
  check_against_a_map(b, process);
  // a failing stream keeps the rows before the stop and writes nothing from it on
  if (steps >= 4) {
    Batch e(S, steps);
    for (uint32_t a = 0; a < steps; ++a) {
      e.rifl[fx_index(a, 0, steps)] = (1u << 24) | (a / 2u);
      e.count[fx_index(a, 0, steps)] = 2;
      e.order[fx_index(a, 0, steps)] = a;
    }
    e.nexec[0] = steps;
    e.order[fx_index(3, 0, steps)] = steps;
    if (S > 1) e.nexec[1] = steps + 1;
    EXPECT(fx_pending_aggregate_host(&e.in, &e.out, FX_PENDING_TIER_ONCHIP) == FX_OK, "aggregate with bad streams");
    EXPECT(e.err[0] == FX_ERR_INVALID_ARG && e.nready[0] == 1 && e.nopen[0] == 1, "status %u, nready %u, nopen %u",
           e.err[0], e.nready[0], e.nopen[0]);
    EXPECT(e.head[fx_index(2, 0, steps)] == 2 && e.head[fx_index(3, 0, steps)] == A5, "the rows around the stop");
    if (S > 1) EXPECT(e.err[1] == FX_ERR_ORDER_OVERFLOW && e.nready[1] == 0 && e.nopen[1] == 0, "status %u", e.err[1]);
  }
}

// 65 commands of two partials, every first half before any second: the ONCHIP
// tier stops at the 65th, the HBM tier completes them all.
void capacity() {
  const uint32_t steps = 130;
  for (uint32_t tier = 0; tier < 2; ++tier) {
    Batch b(1, steps);
    for (uint32_t a = 0; a < steps; ++a) {
      b.rifl[fx_index(a, 0, steps)] = (1u << 24) | (a % 65u);
      b.count[fx_index(a, 0, steps)] = 2;
      b.order[fx_index(a, 0, steps)] = a;
    }
    b.nexec[0] = steps;
    EXPECT(fx_pending_aggregate_host(&b.in, &b.out, tier) == FX_OK, "aggregate");
    if (tier == FX_PENDING_TIER_ONCHIP) {
      EXPECT(b.err[0] == FX_ERR_CAPACITY && b.nopen[0] == 64 && b.nready[0] == 0, "status %u", b.err[0]);
      EXPECT(b.head[fx_index(63, 0, steps)] == 63 && b.head[fx_index(64, 0, steps)] == A5, "the rows around the stop");
    } else {
      EXPECT(b.err[0] == FX_OK && b.nopen[0] == 0 && b.nready[0] == 65, "status %u", b.err[0]);
    }
  }
}

}  // namespace

int main() {
  // (S, steps, process, seed)
  run(1, 1, 0, 1);
  run(1, 131, 0, 2);
  run(64, 66, 2, 3);
  run(65, 130, 0, 4);
  run(3, 7, 1, 5);
  capacity();
  {
    Batch b(2, 8);
    fx_pending_batch in = b.in;
    in.count_mask = 0;
    EXPECT(fx_pending_aggregate_host(&in, &b.out, FX_PENDING_TIER_HBM) == FX_ERR_INVALID_ARG, "count_mask 0 accepted");
    EXPECT(fx_pending_aggregate_host(&b.in, &b.out, 2) == FX_ERR_INVALID_ARG, "tier 2 accepted");
    fx_pending_out out = b.out;
    out.index = nullptr;
    EXPECT(fx_pending_aggregate_host(&b.in, &out, FX_PENDING_TIER_HBM) == FX_ERR_INVALID_ARG, "a null plane accepted");
    EXPECT(b.err[0] == A5 && b.nready[0] == A5 && b.head[0] == A5, "a refused call wrote");
    EXPECT(fx_pending_state_bytes(1, 1) == 1024 && fx_pending_state_bytes(65, 3) == 3 * 2048, "state bytes");
    EXPECT(fx_pending_bucket(12345, 1) == 0 && fx_pending_bucket(12345, 7) < 7, "bucket");
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("pending_host_check: ok\n");
  return 0;
}
