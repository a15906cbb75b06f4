// The host twins of the slot executor (fx_slot_execute_host,
// fx_slot_synth_generate_host) on buffers allocated at exactly the sizes the
// header states (planes of fx_plane_words words, [S] arrays).  Built with
// -fsanitize=address,undefined (`make slot-check`), so a store one word outside
// a buffer, or a read of one, stops the program.  The outputs are also checked
// against a std::map of waiting slots, and the words a call must leave alone
// against their sentinel.  Host only: no device.
#include <stdio.h>

#include <algorithm>
#include <map>
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
  std::vector<uint32_t> slot, lengths, order, release, nexec, err;
  fx_slot_batch in;
  fx_order_batch out;
  Batch(uint32_t S_, uint32_t steps_) : S(S_), steps(steps_) {
    const size_t pw = fx_plane_words(S, steps);
    slot.assign(pw, A5);
    lengths.assign(S, steps);
    order.assign(pw, A5);
    release.assign(pw, A5);
    nexec.assign(S, A5);
    err.assign(S, A5);
    in = fx_slot_batch{slot.data(), lengths.data(), S, steps};
    out = fx_order_batch{order.data(), release.data(), nexec.data(), err.data()};
  }
};

// the executor of slot.rs over a std::map, and every word of the outputs
void check_against_a_map(const Batch& b, bool at_commit) {
  const size_t pw = fx_plane_words(b.S, b.steps);
  std::vector<bool> order_set(pw), release_set(pw);
  for (uint32_t s = 0; s < b.S; ++s) {
    const uint32_t len = std::min(b.lengths[s], b.steps);
    std::map<uint32_t, uint32_t> waiting;
    std::vector<uint32_t> order, release(len, A5);
    uint32_t next = 1, status = FX_OK;
    for (uint32_t a = 0; a < len && !status; ++a) {
      const uint32_t v = b.slot[fx_index(a, s, b.steps)];
      if (at_commit) {
        if (v == 0) {
          status = FX_ERR_SLOT;
        } else {
          order.push_back(a);
          release[a] = a;
        }
        continue;
      }
      if (v < next || waiting.count(v)) status = FX_ERR_SLOT;
      if (v >= next && v > b.steps) status = FX_ERR_CAPACITY;
      if (status) break;
      waiting[v] = a;
      release[a] = FX_RELEASE_NONE;
      while (waiting.count(next)) {
        order.push_back(waiting[next]);
        release[waiting[next]] = a;
        waiting.erase(next++);
      }
    }
    EXPECT(b.err[s] == status, "stream %u: status %u, want %u", s, b.err[s], status);
    EXPECT(b.nexec[s] == order.size(), "stream %u: nexec %u, want %zu", s, b.nexec[s], order.size());
    for (uint32_t k = 0; k < order.size(); ++k) {
      const size_t at = fx_index(k, s, b.steps);
      order_set[at] = true;
      EXPECT(b.order[at] == (order[k] | FX_ORDER_SCC_START), "stream %u: order row %u", s, k);
    }
    for (uint32_t a = 0; a < len; ++a) {
      const size_t at = fx_index(a, s, b.steps);
      release_set[at] = release[a] != A5;
      EXPECT(b.release[at] == release[a], "stream %u: release of row %u: %u, want %u", s, a, b.release[at], release[a]);
    }
  }
  for (size_t w = 0; w < pw; ++w) {
    EXPECT(order_set[w] || b.order[w] == A5, "order word %zu written", w);
    EXPECT(release_set[w] || b.release[w] == A5, "release word %zu written", w);
  }
}

void run(uint32_t S, uint32_t steps, uint32_t window, uint32_t seed) {
  Batch b(S, steps);
  for (uint32_t s = 0; s < S; ++s) b.lengths[s] = (s * 37u + seed) % (steps + 2u);  // some beyond steps: capped
  EXPECT(fx_slot_synth_generate_host(seed, 1000u * seed, S, steps, b.lengths.data(), window, b.slot.data()) == FX_OK,
         "generate");
  // a stream of the generator: every slot 1 .. L once, none displaced by `window` or more, pad words 0
  const size_t pw = fx_plane_words(S, steps);
  std::vector<bool> used(pw);
  for (uint32_t s = 0; s < S; ++s) {
    const uint32_t L = std::min(b.lengths[s], steps);
    std::vector<uint32_t> seen(L + 1u, 0u);
    for (uint32_t a = 0; a < L; ++a) {
      const size_t at = fx_index(a, s, steps);
      const uint32_t v = b.slot[at];
      used[at] = true;
      EXPECT(v >= 1 && v <= L && !seen[std::min(v, L)]++, "stream %u row %u: slot %u", s, a, v);
      EXPECT((v > a + 1 ? v - a - 1 : a + 1 - v) < window, "stream %u row %u: slot %u displaced", s, a, v);
    }
  }
  for (size_t w = 0; w < pw; ++w) EXPECT(used[w] || b.slot[w] == 0u, "pad word %zu is %u", w, b.slot[w]);
  for (uint32_t at_commit = 0; at_commit < 2; ++at_commit) {
    Batch r(S, steps);
    r.slot = b.slot;
    r.lengths = b.lengths;
    r.in.slot = r.slot.data();
    r.in.lengths = r.lengths.data();
    // a few bad rows: slot 0, a repeat, a slot above steps
    if (steps >= 8) {
      r.slot[fx_index(steps / 2u, 0, steps)] = 0u;
      if (S > 1) r.slot[fx_index(steps - 1u, 1, steps)] = r.slot[fx_index(0, 1, steps)];
      if (S > 2) r.slot[fx_index(2, 2, steps)] = steps + 1u;
    }
    EXPECT(fx_slot_execute_host(&r.in, &r.out, at_commit ? FX_FLAG_EXECUTE_AT_COMMIT : 0u) == FX_OK, "execute");
    check_against_a_map(r, at_commit != 0);
  }
}

}  // namespace

int main() {
  // (S, steps, window, seed)
  run(1, 1, 1, 1);
  run(1, 131, 8, 2);
  run(64, 66, 64, 3);
  run(65, 130, 200, 4);
  run(3, 7, 2, 5);
  {
    Batch b(2, 8);
    fx_slot_batch in = b.in;
    in.lengths = nullptr;  // every stream has `steps` rows
    for (uint32_t s = 0; s < 2; ++s)
      for (uint32_t a = 0; a < 8; ++a) b.slot[fx_index(a, s, 8)] = 8u - a;
    EXPECT(fx_slot_execute_host(&in, &b.out, 0) == FX_OK && b.nexec[1] == 8 && b.err[1] == FX_OK, "reversed");
    EXPECT(b.release[fx_index(0, 1, 8)] == 7 && b.order[fx_index(0, 1, 8)] == (7u | FX_ORDER_SCC_START), "reversed rows");
    Batch c(2, 8);
    in = c.in;
    in.slot = nullptr;
    EXPECT(fx_slot_execute_host(&in, &c.out, 0) == FX_ERR_INVALID_ARG, "a null plane accepted");
    EXPECT(fx_slot_execute_host(&c.in, &c.out, FX_FLAG_INIT) == FX_ERR_INVALID_ARG, "an unknown flag accepted");
    fx_order_batch out = c.out;
    out.release = nullptr;
    EXPECT(fx_slot_execute_host(&c.in, &out, 0) == FX_ERR_INVALID_ARG, "a null output accepted");
    EXPECT(c.err[0] == A5 && c.nexec[0] == A5 && c.order[0] == A5, "a refused call wrote");
    EXPECT(fx_slot_synth_generate_host(1, 0, 2, 8, nullptr, 0, c.slot.data()) == FX_ERR_INVALID_ARG, "window 0 accepted");
    EXPECT(fx_slot_state_bytes(1, 1) == 256 && fx_slot_state_bytes(65, 3) == 3 * 512, "state bytes");
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("slot_host_check: ok\n");
  return 0;
}
