// The host twin of the pending stage's sessions (fx_pending_advance_host) on
// buffers allocated at exactly the sizes the header states (planes of
// fx_plane_words words, FX_PENDING_MAX_PARTS part planes, a state of
// fx_pending_session_bytes bytes).  Built with -fsanitize=address,undefined
// (`make pending-advance-check`), so a store one word outside a buffer, or a
// read of one, stops the program.  Random streams (commands of 1 to 4
// partials, some nobody waits for, a few count mismatches) are fed in random
// pieces; after every call every output is compared word for word with
// fx_pending_aggregate_host at the HBM tier over the same nexec on buffers of
// the same initial content.  Host only: no device.
#include <stdio.h>

#include <algorithm>
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

struct Outs {
  std::vector<uint32_t> part, head, ready, index, nready, nopen, err;
  fx_pending_out out;
  Outs(uint32_t S, uint32_t steps)
      : part(FX_PENDING_MAX_PARTS * fx_plane_words(S, steps), A5), head(fx_plane_words(S, steps), A5),
        ready(fx_plane_words(S, steps), A5), index(fx_plane_words(S, steps), A5), nready(S, A5), nopen(S, A5),
        err(S, A5) {
    out = fx_pending_out{part.data(), head.data(), ready.data(), index.data(), nready.data(), nopen.data(), err.data()};
  }
  bool operator==(const Outs& o) const {
    return part == o.part && head == o.head && ready == o.ready && index == o.index && nready == o.nready &&
           nopen == o.nopen && err == o.err;
  }
};

void run(uint32_t S, uint32_t steps, uint32_t process, uint32_t seed) {
  std::mt19937 rng(seed);
  const size_t pw = fx_plane_words(S, steps);
  std::vector<uint32_t> order(pw, A5), rifl(pw, A5), count(pw, A5), nexec(S, 0), full(S);
  for (uint32_t s = 0; s < S; ++s) {
    // commands of 1 .. 4 partials, the partials shuffled a little
    std::vector<std::pair<uint32_t, uint32_t>> rows;
    for (uint32_t c = 0; rows.size() < steps; ++c) {
      const uint32_t n = std::min<uint32_t>(1 + rng() % 4, steps - (uint32_t)rows.size());
      const uint32_t cnt = rng() % 8 == 0 ? 0 : rng() % 97 == 0 ? n + 1 : n;  // a few mismatches stop the stream
      for (uint32_t j = 0; j < n; ++j) rows.push_back({((1 + c % 3) << 24) | (c % 40), cnt});
    }
    for (uint32_t a = 0; a + 1 < steps; ++a)
      if (rng() % 2) std::swap(rows[a], rows[a + rng() % std::min<uint32_t>(8, steps - a)]);
    for (uint32_t a = 0; a < steps; ++a) {
      rifl[fx_index(a, s, steps)] = rows[a].first;
      count[fx_index(a, s, steps)] = rows[a].second | 0x300u;
      order[fx_index(a, s, steps)] = a | (a % 2 ? FX_ORDER_SCC_START : 0u);
    }
    full[s] = steps ? rng() % (steps + 1) : 0;
  }
  Outs ses(S, steps);
  std::vector<uint8_t> state(fx_pending_session_bytes(steps, S), 0xA5);
  const fx_pending_batch in{order.data(), nexec.data(), rifl.data(), count.data(), 0xFFu, process, S, steps};
  bool first = true, finished = false;
  while (!finished) {
    finished = true;
    for (uint32_t s = 0; s < S; ++s) {
      nexec[s] = std::min<uint32_t>(full[s], nexec[s] + rng() % 70);
      finished = finished && nexec[s] == full[s];
    }
    EXPECT(fx_pending_advance_host(&in, &ses.out, state.data(), first ? FX_FLAG_INIT : 0u) == FX_OK, "advance");
    first = false;
    Outs whole(S, steps);
    EXPECT(fx_pending_aggregate_host(&in, &whole.out, FX_PENDING_TIER_HBM) == FX_OK, "aggregate");
    EXPECT(ses == whole, "S %u steps %u process %u seed %u", S, steps, process, seed);
  }
}

}  // namespace

int main() {
  uint32_t seed = 1;
  for (uint32_t S : {1u, 3u, 65u})
    for (uint32_t steps : {1u, 63u, 65u, 200u})
      for (uint32_t process : {0u, 2u}) run(S, steps, process, seed++);
  Outs o(1, 4);
  std::vector<uint32_t> plane(fx_plane_words(1, 4), 0), ne(1, 0);
  std::vector<uint8_t> state(fx_pending_session_bytes(4, 1), 0xA5);
  fx_pending_batch in{plane.data(), ne.data(), plane.data(), plane.data(), 0xFFu, 0, 1, 4};
  EXPECT(fx_pending_advance_host(&in, &o.out, nullptr, FX_FLAG_INIT) == FX_ERR_INVALID_ARG, "null state");
  EXPECT(fx_pending_advance_host(&in, &o.out, state.data(), 4u) == FX_ERR_INVALID_ARG, "flags");
  in.count_mask = 0;
  EXPECT(fx_pending_advance_host(&in, &o.out, state.data(), FX_FLAG_INIT) == FX_ERR_INVALID_ARG, "count_mask 0");
  EXPECT(o.err[0] == A5 && state[0] == 0xA5, "a refused call wrote");
  printf(failures ? "%d FAILED\n" : "pending_advance_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
