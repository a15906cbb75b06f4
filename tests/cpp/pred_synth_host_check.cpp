// The host twin of the Caesar commit-stream generator
// (fx_pred_synth_generate_host) on buffers allocated at exactly the sizes the
// header states (planes of fx_plane_words words, dmax dep planes).  Built with
// -fsanitize=address,undefined (`make pred-synth-check`), so a store one word
// outside a buffer, or a read of one, stops the program.  Shapes A to D of
// tests/pred_synth_shapes.py: the planes must hold every dot once per stream
// with distinct clocks, ascending deps of the same instance, zero fill behind
// them and the poison word in every pad; the same shape as D with one more
// round of history is refused and stores nothing.  Host only: no device.
#include <stdio.h>

#include <algorithm>
#include <set>
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

struct Shape {
  const char* name;
  fx_pred_synth_params p;
  uint32_t S, steps, dmax;
  bool ndeps;
};

fx_pred_synth_params params(uint64_t seed, uint32_t n, uint32_t instances, uint32_t cmds, uint32_t window,
                            uint32_t horizon, uint32_t max_bump, uint32_t retry, std::vector<uint32_t> conflicts) {
  fx_pred_synth_params p{};
  p.seed = seed;
  p.instances = instances;
  p.n = n;
  p.cmds_per_process = cmds;
  p.window = window;
  p.horizon = horizon;
  p.max_bump = max_bump;
  p.retry_pct = retry;
  p.num_conflicts = (uint32_t)conflicts.size();
  for (size_t i = 0; i < conflicts.size(); ++i) p.conflict_pct[i] = conflicts[i];
  return p;
}

struct Buffers {
  std::vector<uint32_t> dot, hdr, deps, clo, chi, nd;
  fx_pred_synth_planes pl;
  Buffers(uint32_t S, uint32_t steps, uint32_t dmax, bool ndeps)
      : dot(fx_plane_words(S, steps), A5), hdr(dot.size(), A5), deps(dot.size() * dmax, A5), clo(dot.size(), A5),
        chi(dot.size(), A5), nd(ndeps ? dot.size() : 0, A5) {
    pl = fx_pred_synth_planes{dot.data(), hdr.data(), deps.data(), clo.data(), chi.data(), ndeps ? nd.data() : nullptr};
  }
  bool untouched() const {
    for (const auto* v : {&dot, &hdr, &deps, &clo, &chi, &nd})
      for (uint32_t x : *v)
        if (x != A5) return false;
    return true;
  }
};

void check(const Shape& sh) {
  uint32_t S = 0, steps = 0, dmax = 0;
  EXPECT(fx_pred_synth_shape(&sh.p, &S, &steps, &dmax) == FX_OK, "%s: shape", sh.name);
  EXPECT(S == sh.S && steps == sh.steps && dmax == sh.dmax, "%s: shape %u %u %u", sh.name, S, steps, dmax);
  Buffers b(sh.S, sh.steps, sh.dmax, sh.ndeps);
  EXPECT(fx_pred_synth_generate_host(&sh.p, &b.pl) == FX_OK, "%s: generate", sh.name);
  const size_t pw = b.dot.size();
  std::vector<char> in_range(pw, 0);
  const uint32_t n = sh.p.n;
  for (uint32_t s = 0; s < S; ++s) {
    std::set<uint32_t> dots;
    std::set<uint64_t> clocks;
    for (uint32_t r = 0; r < steps; ++r) {
      const size_t at = fx_index(r, s, steps);
      in_range[at] = 1;
      const uint32_t d = b.dot[at], nd = sh.ndeps ? b.nd[at] : FX_HDR_ND(b.hdr[at]);
      EXPECT(FX_DOT_SRC(d) >= 1 && FX_DOT_SRC(d) <= n && FX_DOT_SEQ(d) >= 1 && FX_DOT_SEQ(d) <= sh.p.cmds_per_process,
             "%s: dot %08x", sh.name, d);
      dots.insert(d);
      const uint64_t clock = ((uint64_t)b.chi[at] << 32) | b.clo[at];
      clocks.insert(clock);
      EXPECT((clock & 255u) == FX_DOT_SRC(d), "%s: clock id", sh.name);
      EXPECT(FX_HDR_KIND(b.hdr[at]) == FX_KIND_ADD && FX_HDR_ND(b.hdr[at]) == std::min(nd, 31u) && nd <= dmax,
             "%s: header %08x, %u deps", sh.name, b.hdr[at], nd);
      uint32_t prev = 0;
      for (uint32_t k = 0; k < dmax; ++k) {
        const uint32_t x = b.deps[k * pw + at];
        if (k < nd) {
          EXPECT(x > prev && x != d && FX_DOT_SRC(x) >= 1 && FX_DOT_SRC(x) <= n && FX_DOT_SEQ(x) >= 1 &&
                     FX_DOT_SEQ(x) <= sh.p.cmds_per_process,
                 "%s: stream %u row %u dep %u = %08x", sh.name, s, r, k, x);
          prev = x;
        } else {
          EXPECT(x == 0, "%s: stream %u row %u slot %u = %08x", sh.name, s, r, k, x);
        }
      }
    }
    EXPECT(dots.size() == steps && clocks.size() == steps, "%s: stream %u holds %zu dots, %zu clocks", sh.name, s,
           dots.size(), clocks.size());
  }
  size_t pads = 0, touched = 0;
  for (size_t at = 0; at < pw; ++at) {
    if (in_range[at]) continue;
    ++pads;
    touched += b.dot[at] != A5 || b.hdr[at] != A5 || b.clo[at] != A5 || b.chi[at] != A5 || (sh.ndeps && b.nd[at] != A5);
    for (uint32_t k = 0; k < dmax; ++k) touched += b.deps[k * pw + at] != A5;
  }
  EXPECT(pads > 0 && touched == 0, "%s: %zu pad words written", sh.name, touched);
}

}  // namespace

int main() {
  const std::vector<Shape> shapes = {
      {"A", params(11, 5, 3, 3, 2, 1, 0, 30, {100}), 15, 15, 9, false},
      {"B", params(12, 5, 13, 8, 8, 4, 2, 40, {0, 50, 100}), 65, 40, 34, true},
      {"C", params(13, 3, 2, 16, 0, 15, 3, 100, {50, 100}), 6, 48, 56, true},
      {"D", params(14, 8, 1, 2, 8, 28, 3, 30, {50}), 8, 16, 255, true},
  };
  for (const Shape& sh : shapes) check(sh);
  {
    // D with one more round of history: dmax 263
    fx_pred_synth_params p = shapes[3].p;
    p.horizon = 29;
    uint32_t S = 7, steps = 7, dmax = 7;
    EXPECT(fx_pred_synth_shape(&p, &S, &steps, &dmax) == FX_ERR_INVALID_ARG && S == 7 && steps == 7 && dmax == 7,
           "dmax 263: shape");
    Buffers b(8, 16, 255, true);
    EXPECT(fx_pred_synth_generate_host(&p, &b.pl) == FX_ERR_INVALID_ARG && b.untouched(), "dmax 263: generate");
    // ndeps may be NULL up to dmax 31 only
    Buffers c(65, 40, 34, true);
    c.pl.ndeps = nullptr;
    EXPECT(fx_pred_synth_generate_host(&shapes[1].p, &c.pl) == FX_ERR_INVALID_ARG && c.untouched(), "B without ndeps");
    c.pl.ndeps = c.nd.data();
    c.pl.clock_hi = nullptr;
    EXPECT(fx_pred_synth_generate_host(&shapes[1].p, &c.pl) == FX_ERR_INVALID_ARG && c.untouched(), "B without clock_hi");
    EXPECT(fx_pred_synth_generate_host(&shapes[1].p, nullptr) == FX_ERR_INVALID_ARG, "no planes");
    EXPECT(fx_pred_synth_generate_host(nullptr, &c.pl) == FX_ERR_INVALID_ARG, "no params");
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("pred_synth_host_check: ok\n");
  return 0;
}
