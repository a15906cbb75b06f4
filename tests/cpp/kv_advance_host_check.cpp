// The host twins of the KV stage's sessions (fx_kv_advance_host,
// fx_kv_session_monitor_host) on buffers allocated at exactly the sizes the
// header states (planes of fx_plane_words words, [S * keys] stores, a state of
// fx_kv_session_bytes bytes).  Built with -fsanitize=address,undefined (`make
// kv-advance-check`), so a store one word outside a buffer, or a read of one,
// stops the program.  Random streams are fed in random pieces; after every
// call result and store, and after the monitor call monitor, mon_off, store
// and err, are compared word for word with fx_kv_execute_host over the same
// nexec on buffers of the same initial content.  Host only: no device.
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
  std::vector<uint32_t> result, store, monitor, mon_off, rank, err;
  Outs(uint32_t S, uint32_t steps, uint32_t keys, uint32_t omax)
      : result(omax * fx_plane_words(S, steps), A5), store((size_t)S * keys, A5), monitor(fx_plane_words(S, steps), A5),
        mon_off((size_t)S * (keys + 1), A5), rank(fx_plane_words(S, steps), A5), err(S, A5) {}
};

void run(uint32_t S, uint32_t steps, uint32_t keys, uint32_t omax, uint32_t seed) {
  std::mt19937 rng(seed);
  const size_t pw = fx_plane_words(S, steps);
  std::vector<uint32_t> order(pw, A5), key(pw, A5), ops(omax * pw, A5), nexec(S, 0), full(S);
  for (uint32_t s = 0; s < S; ++s) {
    std::vector<uint32_t> rows(steps);
    for (uint32_t a = 0; a < steps; ++a) rows[a] = a;
    std::shuffle(rows.begin(), rows.end(), rng);
    full[s] = steps ? rng() % (steps + 1) : 0;
    for (uint32_t k = 0; k < full[s]; ++k) order[fx_index(k, s, steps)] = rows[k] | (k % 3 ? 0u : FX_ORDER_SCC_START);
    for (uint32_t a = 0; a < steps; ++a) {
      key[fx_index(a, s, steps)] = rng() % keys;
      const uint32_t used = rng() % (omax + 1);
      for (uint32_t j = 0; j < omax; ++j) {
        const uint32_t kind = rng() % 3;
        ops[j * pw + fx_index(a, s, steps)] =
            j < used ? FX_KV_OP(kind, kind == FX_KV_PUT ? 1 + rng() % 1000 : 0) : FX_KV_OP(FX_KV_EMPTY, 0);
      }
    }
  }
  Outs ses(S, steps, keys, omax);
  std::vector<uint8_t> state(fx_kv_session_bytes(keys, S), 0xA5);
  const fx_kv_batch in{order.data(), nexec.data(), key.data(), 0xFFFFFFFFu, ops.data(), S, steps, keys, omax};
  const fx_kv_session_out sout{ses.result.data(), ses.store.data(), ses.rank.data(), ses.err.data()};
  bool first = true, finished = false;
  while (!finished) {
    finished = true;
    for (uint32_t s = 0; s < S; ++s) {
      nexec[s] = std::min<uint32_t>(full[s], nexec[s] + rng() % 70);
      finished = finished && nexec[s] == full[s];
    }
    EXPECT(fx_kv_advance_host(&in, &sout, state.data(), first ? FX_FLAG_INIT : 0u) == FX_OK, "advance");
    first = false;
    Outs whole(S, steps, keys, omax), mon(S, steps, keys, omax);
    const fx_kv_out wout{whole.result.data(), whole.store.data(), whole.monitor.data(), whole.mon_off.data(),
                         whole.err.data()};
    EXPECT(fx_kv_execute_host(&in, &wout) == FX_OK, "execute");
    EXPECT(ses.result == whole.result && ses.store == whole.store && ses.err == whole.err, "S %u steps %u keys %u", S,
           steps, keys);
    const fx_kv_out mout{ses.result.data(), mon.store.data(), mon.monitor.data(), mon.mon_off.data(), mon.err.data()};
    EXPECT(fx_kv_session_monitor_host(&in, ses.rank.data(), &mout, state.data()) == FX_OK, "monitor");
    EXPECT(mon.monitor == whole.monitor && mon.mon_off == whole.mon_off && mon.store == whole.store &&
               mon.err == whole.err,
           "monitor: S %u steps %u keys %u", S, steps, keys);
  }
}

}  // namespace

int main() {
  uint32_t seed = 1;
  for (uint32_t S : {1u, 3u, 65u})
    for (uint32_t steps : {1u, 63u, 130u})
      for (uint32_t keys : {1u, 65u, 600u})
        for (uint32_t omax : {1u, 4u}) run(S, steps, keys, omax, seed++);
  // refusals touch nothing
  Outs o(1, 4, 2, 1);
  std::vector<uint32_t> plane(fx_plane_words(1, 4), 0), ne(1, 0);
  std::vector<uint8_t> state(fx_kv_session_bytes(2, 1), 0xA5);
  fx_kv_batch in{plane.data(), ne.data(), plane.data(), 0xFFFFFFFFu, plane.data(), 1, 4, 2, 1};
  fx_kv_session_out out{o.result.data(), o.store.data(), o.rank.data(), o.err.data()};
  EXPECT(fx_kv_advance_host(&in, &out, nullptr, FX_FLAG_INIT) == FX_ERR_INVALID_ARG, "null state");
  EXPECT(fx_kv_advance_host(&in, &out, state.data(), 2u) == FX_ERR_INVALID_ARG, "flags");
  out.rank = nullptr;
  EXPECT(fx_kv_advance_host(&in, &out, state.data(), FX_FLAG_INIT) == FX_ERR_INVALID_ARG, "null rank");
  EXPECT(o.err[0] == A5 && state[0] == 0xA5, "a refused call wrote");
  printf(failures ? "%d FAILED\n" : "kv_advance_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
