// The host twin of the metrics pass (fx_batch_metrics_host) on buffers allocated
// at exactly the sizes the header states (planes of fx_plane_words words, nexec
// of S words, histograms of nbins words).  Built with
// -fsanitize=address,undefined (`make metrics-check`), so a read of one word
// outside a plane, or a count added one bin outside a histogram, stops the
// program.  Every word the call must not read holds 0xA5 bytes.  The histograms
// are also checked against a forward scan written here: it closes an SCC when
// the next flagged row or the end of the stream comes, where the twin and the
// kernel walk ahead from the flagged row.  The cases follow
// tests/metrics_edges.py; one more, which only the host may run, has the
// counts of streams no launch wrote (0xA5A5A5A5).  Host only: no device.
#include <stdio.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "fantoch_amd.h"

namespace {

int failures = 0;
constexpr uint32_t A5 = 0xA5A5A5A5u;
constexpr uint32_t STALE = 0x25A5A5A5u;  // the fill without the flag
constexpr uint32_t BASE = 0x800000u, T_MAX = 0xFFFFFFu;
constexpr uint32_t LDS_WORDS = 48u * 1024u / 4u;
const uint32_t PAIRS[4][2] = {{2, 2}, {64, 4096}, {64, LDS_WORDS - 64}, {64, LDS_WORDS - 63}};

#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      ++failures;                         \
      printf("FAILED %s: ", #cond);       \
      printf(__VA_ARGS__);                \
      printf("\n");                       \
    }                                     \
  } while (0)

uint64_t rng_state = 1;
uint32_t rnd(uint32_t below) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((rng_state >> 33) % below);
}

struct Planes {
  uint32_t S, steps;
  std::vector<uint32_t> hdr, order, release, nexec;
  Planes(uint32_t S_, uint32_t steps_) : S(S_), steps(steps_) {
    const size_t pw = fx_plane_words(S, steps);
    hdr.assign(pw, A5);
    order.assign(pw, A5);
    release.assign(pw, A5);
    nexec.assign(S, A5);
  }
  size_t at(uint32_t row, uint32_t s) const { return fx_index(row, s, steps); }
  uint32_t hi(uint32_t row, uint32_t s) const { return ((row * 37u + s * 11u + 1u) & 0xFFu) << 24; }
  // stream s executed rec.size() rows: order row k is arrival rec[k] with the delay delays[k]; an arrival
  // releases at its anchor row min(a | 15, steps - 1) (time BASE), an anchor at itself (delay 0)
  void stream(uint32_t s, const std::vector<uint32_t>& rec, const std::vector<bool>& flags,
              const std::vector<int64_t>& delays) {
    for (size_t k = 0; k < rec.size(); ++k) {
      const uint32_t a = rec[k], anchor = std::min(a | 15u, steps - 1u);
      hdr[at(anchor, s)] = BASE | hi(anchor, s);
      if (a != anchor) hdr[at(a, s)] = (uint32_t)((int64_t)BASE - delays[k]) | hi(a, s);
      release[at(a, s)] = anchor;
      order[at((uint32_t)k, s)] = a | (flags[k] ? FX_ORDER_SCC_START : 0u);
    }
    nexec[s] = (uint32_t)rec.size();
  }
  void random_stream(uint32_t s, uint32_t ne) {
    static const int64_t palette[] = {0, 0, 0, 1, 1, 2, 3, 5, 62, 63, 64, 4094, 4095, 4096, LDS_WORDS - 66,
                                      LDS_WORDS - 65, LDS_WORDS - 64, LDS_WORDS - 63, -1};
    std::vector<uint32_t> rec(steps);
    for (uint32_t a = 0; a < steps; ++a) rec[a] = a;
    for (uint32_t a = steps; a > 1; --a) std::swap(rec[a - 1], rec[rnd(a)]);
    rec.resize(ne);
    std::vector<bool> flags(ne);
    std::vector<int64_t> delays(ne);
    for (uint32_t k = 0; k < ne; ++k) {
      flags[k] = rnd(10) < 6;
      delays[k] = palette[rnd(sizeof(palette) / sizeof(palette[0]))];
    }
    stream(s, rec, flags, delays);
  }
};

struct Hists {
  std::vector<uint64_t> chain, delay;
  Hists(uint32_t nbc, uint32_t nbd, bool started) : chain(nbc, 0), delay(nbd, 0) {
    const uint64_t start[3] = {1ull, 0xFFFFFFFFull, 1ull << 40};
    if (started) {
      for (uint32_t q = 0; q < nbc; ++q) chain[q] = start[q % 3];
      for (uint32_t q = 0; q < nbd; ++q) delay[q] = start[(q + 1) % 3];
    }
  }
};

// the forward scan
void scan(const Planes& p, Hists& h) {
  const uint32_t nbc = (uint32_t)h.chain.size(), nbd = (uint32_t)h.delay.size();
  for (uint32_t s = 0; s < p.S; ++s) {
    if (p.nexec[s] > p.steps) continue;
    bool open = false;  // inside an SCC whose first row gave a delay sample
    uint64_t size = 0;
    auto close = [&]() {
      if (open) ++h.chain[std::min<uint64_t>(size, nbc - 1u)];
      open = false;
    };
    for (uint32_t k = 0; k < p.nexec[s]; ++k) {
      const uint32_t o = p.order[p.at(k, s)], rec = o & 0x7FFFFFFFu;
      bool sample = false;
      if (rec < p.steps && p.release[p.at(rec, s)] < p.steps) {
        const uint32_t rs = p.release[p.at(rec, s)];
        const int64_t d = (int64_t)(p.hdr[p.at(rs, s)] & T_MAX) - (int64_t)(p.hdr[p.at(rec, s)] & T_MAX);
        ++h.delay[std::min<uint64_t>(d < 0 ? (uint64_t)(d + (1ll << 32)) : (uint64_t)d, nbd - 1u)];
        sample = true;
      }
      if (o >> 31) {
        close();
        open = sample;
        size = 1;
      } else {
        ++size;
      }
    }
    close();
  }
}

int call(const Planes& p, Hists& h) {
  // copies of exactly the stated sizes on the heap (no spare capacity; no word at all for an empty batch)
  auto exact = [](const std::vector<uint32_t>& v) {
    std::unique_ptr<uint32_t[]> c(new uint32_t[v.size()]);
    std::copy(v.begin(), v.end(), c.get());
    return c;
  };
  const auto hdr = exact(p.hdr), order = exact(p.order), release = exact(p.release), nexec = exact(p.nexec);
  fx_stream_batch in{nullptr, hdr.get(), nullptr, nullptr, p.S, p.steps, 0, 0};
  fx_order_batch out{order.get(), release.get(), nexec.get(), nullptr};
  fx_hist_batch hb{h.chain.data(), (uint32_t)h.chain.size(), h.delay.data(), (uint32_t)h.delay.size()};
  return fx_batch_metrics_host(&in, &out, &hb);
}

// the twin against the scan at every bin pair, from zero and from bins that hold something, twice
void check(const char* what, const Planes& p) {
  for (const auto& pair : PAIRS) {
    for (int started = 0; started < 2; ++started) {
      Hists got(pair[0], pair[1], started != 0), want(pair[0], pair[1], started != 0);
      for (int round = 0; round < 2; ++round) {
        EXPECT(call(p, got) == FX_OK, "%s: status", what);
        scan(p, want);
        EXPECT(got.chain == want.chain, "%s (%u, %u) start %d call %d: ChainSize differs", what, pair[0], pair[1],
               started, round);
        EXPECT(got.delay == want.delay, "%s (%u, %u) start %d call %d: ExecutionDelay differs", what, pair[0],
               pair[1], started, round);
      }
    }
  }
}

std::vector<bool> flags_of(const std::vector<uint32_t>& sizes, uint32_t rows, uint32_t lead = 0) {
  std::vector<bool> f(rows, false);
  uint32_t at = lead;
  for (uint32_t z : sizes) {
    f[at] = true;
    at += z;
  }
  EXPECT(at == rows, "flags_of: %u rows, want %u", at, rows);
  return f;
}

std::vector<uint32_t> iota(uint32_t n) {
  std::vector<uint32_t> v(n);
  for (uint32_t i = 0; i < n; ++i) v[i] = i;
  return v;
}

void shapes() {
  const uint32_t list[][2] = {{1, 1}, {1, 3}, {3, 5}, {5, 7}, {63, 4}, {64, 28}, {64, 32}, {1, 2048}, {64, 40},
                              {65, 40}, {129, 9}, {130, 9}, {64, 8197}, {65, 4101}};
  for (const auto& sh : list) {
    Planes p(sh[0], sh[1]);
    for (uint32_t s = 0; s < p.S; ++s) p.random_stream(s, s % 3 == 0 ? p.steps : rnd(p.steps + 1u));
    char what[64];
    snprintf(what, sizeof what, "shape %ux%u", sh[0], sh[1]);
    check(what, p);
  }
}

void clamps() {
  for (const auto& pair : PAIRS) {
    const uint32_t nbc = pair[0], nbd = pair[1];
    Planes d(4, 16);  // delays nbd - 2, nbd - 1, nbd, 0, 0xFFFFFF and a release earlier than the arrival
    const uint32_t wanted[5] = {nbd - 2, nbd - 1, nbd, 0, T_MAX};
    for (uint32_t s = 0; s < 4; ++s) {
      for (uint32_t a = 0; a < 5; ++a) {
        d.hdr[d.at(a, s)] = (T_MAX - wanted[a]) | 0xFF000000u;
        d.release[d.at(a, s)] = 15;
        d.order[d.at((a + s) % 7, s)] = a | (s & 1 ? 0u : FX_ORDER_SCC_START);
      }
      d.hdr[d.at(15, s)] = T_MAX | 0xFF000000u;
      d.release[d.at(15, s)] = 15;
      d.hdr[d.at(14, s)] = (s < 2 ? 1u : T_MAX) | 0xFF000000u;
      d.release[d.at(14, s)] = 4;  // arrival 4 has time 0
      d.order[d.at((5 + s) % 7, s)] = 14 | FX_ORDER_SCC_START;
      d.order[d.at((6 + s) % 7, s)] = 15;
      d.nexec[s] = 7;
    }
    check("delay clamp", d);
    const uint32_t steps = nbc + 6;
    Planes c(6, steps);
    const std::vector<int64_t> small(steps, 1);
    c.stream(0, iota(steps), flags_of({steps}, steps), small);
    c.stream(1, iota(steps), flags_of({nbc + 3}, steps, 3), small);
    c.stream(2, iota(steps), flags_of({4, nbc, 2}, steps), small);
    std::vector<uint32_t> ones(steps - (nbc - 2), 1);
    if (nbc > 2) ones.insert(ones.begin(), nbc - 2);
    c.stream(3, iota(steps), flags_of(ones, steps), small);
    ones.assign(steps - nbc, 1);
    ones.insert(ones.begin(), nbc - 1);
    c.stream(4, iota(steps), flags_of(ones, steps, 1), small);
    c.stream(5, iota(steps - 2), flags_of({1, nbc, 3}, steps - 2), small);  // an SCC that nexec cuts short
    c.order[c.at(steps - 2, 5)] = c.order[c.at(steps - 1, 5)] = STALE;
    check("chain clamp", c);
  }
}

void rows_that_do_not_count() {
  const uint32_t steps = 21;
  Planes p(8, steps);
  const std::vector<int64_t> d(steps, 2);
  p.nexec[0] = 0;
  p.stream(1, {5}, {true}, {3});
  p.random_stream(2, steps);
  p.stream(3, iota(steps), flags_of({2, 3, 4, 5, 3, 4}, steps), d);  // on flagged rows
  p.order[p.at(2, 3)] = steps | FX_ORDER_SCC_START;
  p.order[p.at(5, 3)] = 0xFFFFFFFFu;
  p.release[p.at(9, 3)] = FX_RELEASE_NONE;
  p.release[p.at(14, 3)] = steps;
  p.order[p.at(17, 3)] = 0x40000000u | 17u | FX_ORDER_SCC_START;  // no row 17, this: all 31 bits are the index
  p.stream(4, iota(steps), flags_of({10, 11}, steps), d);  // on unflagged ones
  p.order[p.at(1, 4)] = steps;
  p.order[p.at(3, 4)] = 0x7FFFFFFFu;
  p.release[p.at(11, 4)] = FX_RELEASE_NONE;
  p.release[p.at(13, 4)] = steps;
  p.order[p.at(15, 4)] = 0x40000000u | 15u;
  p.stream(5, iota(steps), flags_of(std::vector<uint32_t>(steps, 1), steps), d);
  p.nexec[5] = steps + 1;  // no count: nothing from this stream
  p.stream(6, iota(steps), flags_of(std::vector<uint32_t>(steps, 1), steps), d);
  p.nexec[6] = A5;  // the count of a stream no launch wrote
  p.stream(7, iota(steps), flags_of(std::vector<uint32_t>(steps, 1), steps), d);
  p.nexec[7] = 0xFFFFFFFFu;
  check("rows that do not count", p);
  Hists h(64, 4096, false);
  EXPECT(call(p, h) == FX_OK, "status");
  uint64_t samples = 0;
  for (uint64_t v : h.delay) samples += v;
  // streams 1 .. 4: 1 + 21 + (21 - 5) + (21 - 5)
  EXPECT(samples == 54, "%llu delay samples, want 54", (unsigned long long)samples);
}

void empty_and_refused() {
  const uint32_t none[2][2] = {{0, 8}, {8, 0}};
  for (const auto& sh : none) {
    Planes p(sh[0], sh[1]);
    Hists got(2, 2, true), want(2, 2, true);
    EXPECT(call(p, got) == FX_OK && got.chain == want.chain && got.delay == want.delay, "empty %ux%u", sh[0], sh[1]);
  }
  Planes p(2, 8);
  p.random_stream(0, 8);
  p.random_stream(1, 3);
  Hists h(4, 4, true), before(4, 4, true);
  const fx_stream_batch in{nullptr, p.hdr.data(), nullptr, nullptr, 2, 8, 0, 0};
  const fx_order_batch out{p.order.data(), p.release.data(), p.nexec.data(), nullptr};
  const fx_hist_batch hb{h.chain.data(), 4, h.delay.data(), 4};
  const int bad = FX_ERR_INVALID_ARG;
  EXPECT(fx_batch_metrics_host(nullptr, &out, &hb) == bad, "null batch");
  EXPECT(fx_batch_metrics_host(&in, nullptr, &hb) == bad, "null outputs");
  EXPECT(fx_batch_metrics_host(&in, &out, nullptr) == bad, "null histograms");
  fx_stream_batch i2 = in;
  i2.hdr = nullptr;
  EXPECT(fx_batch_metrics_host(&i2, &out, &hb) == bad, "null hdr");
  for (int f = 0; f < 3; ++f) {
    fx_order_batch o2 = out;
    (f == 0 ? o2.order : f == 1 ? o2.release : o2.nexec) = nullptr;
    EXPECT(fx_batch_metrics_host(&in, &o2, &hb) == bad, "null output %d", f);
  }
  for (int f = 0; f < 6; ++f) {
    fx_hist_batch h2 = hb;
    if (f == 0) h2.chain_size = nullptr;
    if (f == 1) h2.execution_delay = nullptr;
    if (f == 2 || f == 3) h2.nbins_chain = f - 2;
    if (f == 4 || f == 5) h2.nbins_delay = f - 4;
    EXPECT(fx_batch_metrics_host(&in, &out, &h2) == bad, "bad histogram %d", f);
  }
  EXPECT(h.chain == before.chain && h.delay == before.delay, "a refused call wrote");
  EXPECT(fx_batch_metrics_host(&in, &out, &hb) == FX_OK && h.delay != before.delay, "the valid call");
}

}  // namespace

int main() {
  shapes();
  clamps();
  rows_that_do_not_count();
  empty_and_refused();
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("metrics_host_check: ok\n");
  return 0;
}
