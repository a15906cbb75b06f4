// The host twin of the slot executor's sessions (fx_slot_advance_host) on
// buffers allocated at exactly the sizes the header states (planes of
// fx_plane_words words, [S] arrays, a state of fx_slot_session_bytes bytes).
// Built with -fsanitize=address,undefined (`make slot-advance-check`), so a
// store one word outside a buffer, or a read of one, stops the program.  After
// every call of a session every output word is compared with what one
// fx_slot_execute_host with that call's lengths leaves on buffers of 0xA5.
// Host only: no device.
#include <stdio.h>

#include <algorithm>
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

struct Out {
  std::vector<uint32_t> order, release, nexec, err;
  fx_order_batch b;
  Out(uint32_t S, uint32_t steps)
      : order(fx_plane_words(S, steps), A5), release(fx_plane_words(S, steps), A5), nexec(S, A5), err(S, A5) {
    b = fx_order_batch{order.data(), release.data(), nexec.data(), err.data()};
  }
  bool operator==(const Out& o) const {
    return order == o.order && release == o.release && nexec == o.nexec && err == o.err;
  }
};

struct Session {
  uint32_t S, steps, flags;
  std::vector<uint32_t> slot, lengths;
  std::vector<unsigned char> state;
  Out out;
  Session(const std::vector<std::vector<uint32_t>>& streams, uint32_t steps_, uint32_t flags_)
      : S((uint32_t)streams.size()), steps(steps_), flags(flags_), slot(fx_plane_words(S, steps), A5), lengths(S, 0u),
        state(fx_slot_session_bytes(steps, S), 0xA5), out(S, steps) {
    for (uint32_t s = 0; s < S; ++s)
      for (uint32_t a = 0; a < streams[s].size(); ++a) slot[fx_index(a, s, steps)] = streams[s][a];
  }
  int advance(const std::vector<uint32_t>& lens, bool init, uint32_t call_steps = 0) {
    lengths = lens;
    const fx_slot_batch in{slot.data(), lengths.data(), S, call_steps ? call_steps : steps};
    return fx_slot_advance_host(&in, &out.b, state.data(), flags | (init ? FX_FLAG_INIT : 0u));
  }
  // one whole-stream run with the same lengths on buffers of 0xA5
  void check(const char* what, uint32_t call) {
    Out whole(S, steps);
    const fx_slot_batch in{slot.data(), lengths.data(), S, steps};
    EXPECT(fx_slot_execute_host(&in, &whole.b, flags) == FX_OK, "%s: the whole run", what);
    EXPECT(out == whole, "%s: call %u differs from the whole run", what, call);
  }
};

// every stream cut at the same rows: one call per cut
void run_cuts(const char* what, const std::vector<std::vector<uint32_t>>& streams, uint32_t steps, uint32_t flags,
              const std::vector<uint32_t>& cuts) {
  Session x(streams, steps, flags);
  for (uint32_t c = 0; c < cuts.size(); ++c) {
    std::vector<uint32_t> lens(x.S);
    for (uint32_t s = 0; s < x.S; ++s) lens[s] = std::min<uint32_t>(cuts[c], (uint32_t)streams[s].size());
    EXPECT(x.advance(lens, c == 0) == FX_OK, "%s: call %u", what, c);
    x.check(what, c);
  }
}

std::vector<uint32_t> every_row(uint32_t rows) {
  std::vector<uint32_t> cuts;
  for (uint32_t r = 0; r <= rows; ++r) cuts.push_back(r);
  return cuts;
}

}  // namespace

int main() {
  // the reversed stream of 130 slots, one row per call: the last row drains all 130
  std::vector<uint32_t> reversed;
  for (uint32_t k = 130; k >= 1; --k) reversed.push_back(k);
  run_cuts("reversed", {reversed, reversed}, 130, 0, every_row(130));
  run_cuts("reversed at commit", {reversed}, 130, FX_FLAG_EXECUTE_AT_COMMIT, every_row(130));
  // the failing streams (slot 0, repeats of executed and of waiting slots, a slot above steps), cut at every row
  std::vector<uint32_t> long_one;
  for (uint32_t k = 1; k <= 75; ++k) long_one.push_back(k);
  long_one.push_back(81);
  long_one.push_back(76);
  const std::vector<std::vector<uint32_t>> errors = {
      {0, 1, 2}, {2, 1, 3, 0, 4, 5}, {1, 2, 3, 2, 4}, {1, 3, 5, 3, 2, 4}, {1, 70, 2, 2, 3}, {1, 2, 81, 3},
      long_one,  {1, 0, 3, 3},       {1, 3, 3, 0},    {2, 81, 2, 0, 1},   {5, 4, 6, 1, 2, 2, 3}};
  run_cuts("errors", errors, 80, 0, every_row(77));
  run_cuts("errors at commit", errors, 80, FX_FLAG_EXECUTE_AT_COMMIT, every_row(77));
  run_cuts("errors in three calls", errors, 80, 0, {2, 4, 80});
  {
    // a bad header: a state that never saw FX_FLAG_INIT, other steps, the other commit flag
    Session x({{2, 1, 3}, {1, 2, 3}}, 8, 0);
    const std::vector<unsigned char> raw = x.state;
    EXPECT(x.advance({3, 3}, false) == FX_OK, "a call on a raw state");
    EXPECT(x.out.err[0] == FX_ERR_INVALID_ARG && x.out.err[1] == FX_ERR_INVALID_ARG, "a raw state accepted");
    EXPECT(x.out.nexec[0] == A5 && x.out.order[0] == A5 && x.out.release[0] == A5 && x.state == raw,
           "a call on a raw state wrote");
    EXPECT(x.advance({2, 1}, true) == FX_OK, "init");
    x.check("bad header", 0);
    const std::vector<unsigned char> kept = x.state;
    EXPECT(x.advance({3, 3}, false, 7) == FX_OK && x.out.err[0] == FX_ERR_INVALID_ARG && x.state == kept, "other steps");
    x.flags = FX_FLAG_EXECUTE_AT_COMMIT;
    EXPECT(x.advance({3, 3}, false) == FX_OK && x.out.err[1] == FX_ERR_INVALID_ARG && x.state == kept, "other commit flag");
    x.flags = 0;
    // len < done, then the rest
    EXPECT(x.advance({1, 1}, false) == FX_OK && x.out.err[0] == FX_ERR_INVALID_ARG && x.out.err[1] == FX_OK &&
               x.out.nexec[0] == 2 && x.state == kept,
           "a shorter length");
    EXPECT(x.advance({3, 3}, false) == FX_OK, "the rest");
    x.check("bad header", 1);
    // refusals
    fx_slot_batch in{x.slot.data(), x.lengths.data(), 2, 8};
    const Out before = x.out;
    const std::vector<unsigned char> state_before = x.state;
    EXPECT(fx_slot_advance_host(&in, &x.out.b, nullptr, FX_FLAG_INIT) == FX_ERR_INVALID_ARG, "a null state accepted");
    EXPECT(fx_slot_advance_host(nullptr, &x.out.b, x.state.data(), 0) == FX_ERR_INVALID_ARG, "a null batch accepted");
    EXPECT(fx_slot_advance_host(&in, &x.out.b, x.state.data(), FX_FLAG_SAVE_STATE) == FX_ERR_INVALID_ARG,
           "an unknown flag accepted");
    in.steps = 1u << 31;
    EXPECT(fx_slot_advance_host(&in, &x.out.b, x.state.data(), 0) == FX_ERR_INVALID_ARG, "steps 2^31 accepted");
    in.steps = 8;
    in.slot = nullptr;
    EXPECT(fx_slot_advance_host(&in, &x.out.b, x.state.data(), 0) == FX_ERR_INVALID_ARG, "a null plane accepted");
    EXPECT(x.out == before && x.state == state_before,"a refused call wrote");
    EXPECT(fx_slot_session_bytes(8, 2) >= 2u * (6u + 8u) * 4u, "session bytes");
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("slot_advance_host_check: ok\n");
  return 0;
}
