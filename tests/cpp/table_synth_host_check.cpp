// The host twin of the Tempo stream generator (fx_table_synth_generate_host)
// on planes allocated at exactly fx_plane_words words each, for the edge
// shapes of tests/test_table_synth_cpu.py.  Built with
// -fsanitize=address,undefined (`make synth-check`), so a store one word
// outside a plane, or a read of one, stops the program.  Every plane also
// carries the checks a sanitizer cannot make: rows at or past a stream's
// length are zero, a stream's rows below it are not, and a call that is
// refused leaves its sentinel-filled planes alone.  Host only: no device.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "fantoch_amd.h"

namespace {

int failures = 0;

#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      ++failures;                         \
      printf("FAILED %s: ", #cond);       \
      printf(__VA_ARGS__);                \
      printf("\n");                       \
    }                                     \
  } while (0)

struct Planes {
  std::vector<uint32_t> hdr, dot, clock, votes, nkeys, lengths;
  fx_table_synth_planes c;
  Planes(uint32_t S, uint32_t steps, uint32_t vmax, bool with_nkeys, uint32_t fill) {
    const size_t pw = fx_plane_words(S, steps);
    hdr.assign(pw, fill);
    dot.assign(pw, fill);
    clock.assign(pw, fill);
    votes.assign(pw * 3 * vmax, fill);
    if (with_nkeys) nkeys.assign(pw, fill);
    lengths.assign(S, fill);
    c = fx_table_synth_planes{hdr.data(), dot.data(), clock.data(), votes.data(),
                              with_nkeys ? nkeys.data() : nullptr, lengths.data()};
  }
  bool all(uint32_t v) const {
    for (const auto* p : {&hdr, &dot, &clock, &votes, &nkeys, &lengths})
      for (uint32_t w : *p)
        if (w != v) return false;
    return true;
  }
};

fx_table_synth_params params(uint32_t S, uint32_t n, uint32_t fq, uint32_t keys, uint32_t kmax, uint32_t cmds,
                             uint32_t window, uint32_t lag, uint32_t c0, uint32_t c1, uint32_t block) {
  fx_table_synth_params p{};
  p.seed = 11;
  p.streams = S;
  p.stream_base = 5;
  p.n = n;
  p.fast_quorum = fq;
  p.keys = keys;
  p.cmds = cmds;
  p.kmax = kmax;
  p.window = window;
  p.lag = lag;
  p.num_conflicts = 2;
  p.conflict_pct[0] = c0;
  p.conflict_pct[1] = c1;
  p.conflict_block = block;
  return p;
}

void run(const fx_table_synth_params& p) {
  uint32_t bound = 0, vmax = 0, longest = 0;
  EXPECT(fx_table_synth_shape(&p, &bound, &vmax) == FX_OK, "shape");
  std::vector<uint32_t> len(p.streams);
  EXPECT(fx_table_synth_lengths_host(&p, len.data(), &longest) == FX_OK, "lengths");
  EXPECT(longest <= bound && vmax == p.fast_quorum, "longest %u bound %u vmax %u", longest, bound, vmax);
  // too small by one row: refused, nothing written
  if (longest > 0) {
    Planes small(p.streams, longest - 1, vmax, p.kmax > 1, 0xA5A5A5A5u);
    EXPECT(fx_table_synth_generate_host(&p, &small.c, longest - 1) == FX_ERR_CAPACITY, "capacity");
    EXPECT(small.all(0xA5A5A5A5u), "planes written by a refused call");
  }
  // the exact fit and a fit with spare rows
  for (uint32_t steps : {longest ? longest : 1u, longest + 3}) {
    Planes pl(p.streams, steps, vmax, p.kmax > 1, 0xA5A5A5A5u);
    EXPECT(fx_table_synth_generate_host(&p, &pl.c, steps) == FX_OK, "generate, %u steps", steps);
    const size_t pw = fx_plane_words(p.streams, steps);
    const uint32_t spad = (p.streams + 63u) / 64u * 64u, rows = (steps + 3u) / 4u * 4u;
    for (uint32_t s = 0; s < spad; ++s) {
      const uint32_t L = s < p.streams ? pl.lengths[s] : 0;
      if (s < p.streams) EXPECT(L == len[s], "stream %u: %u events, counted %u", s, L, len[s]);
      for (uint32_t r = 0; r < rows; ++r) {
        const size_t at = fx_index(r, s, steps);
        if (r < L) {
          const uint32_t nv = FX_TABLE_HDR_NVOTES(pl.hdr[at]);
          EXPECT(nv >= 1 && nv <= vmax && pl.votes[at] >= 1 && pl.votes[at] <= p.n &&
                     pl.votes[pw + at] >= 1 && pl.votes[pw + at] <= pl.votes[2 * pw + at],
                 "stream %u row %u: malformed event", s, r);
        } else {
          bool zero = pl.hdr[at] == 0 && pl.dot[at] == 0 && pl.clock[at] == 0 && (pl.nkeys.empty() || pl.nkeys[at] == 0);
          for (uint32_t j = 0; j < 3 * vmax; ++j) zero = zero && pl.votes[j * pw + at] == 0;
          EXPECT(zero, "stream %u row %u past the length %u is not zero", s, r, L);
        }
      }
    }
  }
}

}  // namespace

int main() {
  // (S, n, fq, keys, kmax, cmds, window, lag, conflict rates, conflict_block)
  run(params(1, 3, 2, 1, 1, 40, 0, 0, 0, 100, 0));
  run(params(65, 5, 3, 16, 2, 40, 4, 6, 2, 50, 32));
  run(params(65, 5, 3, 16, 1, 37, 50, 80, 2, 100, 1));
  run(params(2, 7, 4, 2, 2, 60, 9, 3, 100, 0, 0));
  run(params(3, 16, 9, 33, 3, 30, 4, 6, 10, 2, 2));
  run(params(130, 5, 3, 64, 8, 20, 4, 6, 2, 50, 0));
  run(params(4, 5, 3, 16, 2, 0, 4, 6, 2, 2, 0));
  run(params(4, 5, 5, 16, 2, 1, 4, 6, 2, 2, 0));
  // refused arguments leave the planes alone
  {
    fx_table_synth_params bad[] = {params(1, 17, 3, 16, 1, 10, 4, 6, 2, 2, 0), params(1, 5, 6, 16, 1, 10, 4, 6, 2, 2, 0),
                                   params(1, 5, 0, 16, 1, 10, 4, 6, 2, 2, 0), params(1, 5, 3, 16, 9, 10, 4, 6, 2, 2, 0),
                                   params(1, 5, 3, 0, 1, 10, 4, 6, 2, 2, 0),
                                   params(1, 5, 3, FX_TABLE_SYNTH_MAX_KEYS + 1u, 1, 10, 4, 6, 2, 2, 0),
                                   params(1, 5, 3, 16, 1, FX_SEQ_MASK + 1u, 4, 6, 2, 2, 0),
                                   params(1, 5, 3, 16, 1, 10, 4, 6, 101, 2, 0)};
    for (const auto& p : bad) {
      Planes pl(1, 64, 5, true, 0x5A5A5A5Au);
      EXPECT(fx_table_synth_generate_host(&p, &pl.c, 64) == FX_ERR_INVALID_ARG, "bad arguments accepted");
      EXPECT(pl.all(0x5A5A5A5Au), "planes written by a refused call");
      EXPECT(fx_table_synth_shape(&p, nullptr, nullptr) == FX_ERR_INVALID_ARG, "shape of bad arguments");
    }
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("table_synth_host_check: ok\n");
  return 0;
}
