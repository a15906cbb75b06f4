// The host twin of the generator of closed-loop shard groups
// (fx_table_group_synth_generate_host) over the geometries of
// tests/table_group_synth_shapes.py, every buffer allocated at exactly the
// words the call may touch plus a guard word on either side.  Built with
// -fsanitize=address,undefined (`make group-synth-check`): a store outside a
// buffer's allocation stops the program, a store to a guard word fails the
// check below.  Beside that: rows at or past a stream's length are zero
// (route: FX_TABLE_ROUTE_NONE), every list lies inside targets and names
// shards of the group, and a refused call leaves its buffers alone.  Host
// only: no device.
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

constexpr uint32_t GUARD = 0xC3C3C3C3u;

// `words` words between two guard words
struct Guarded {
  std::vector<uint32_t> v;
  Guarded(size_t words, uint32_t fill) : v(words + 2, fill) { v.front() = v.back() = GUARD; }
  uint32_t* data() { return v.data() + 1; }
  const uint32_t& operator[](size_t i) const { return v[i + 1]; }
  size_t size() const { return v.size() - 2; }
  bool guards() const { return v.front() == GUARD && v.back() == GUARD; }
  bool all(uint32_t x) const {
    for (size_t i = 0; i < size(); ++i)
      if ((*this)[i] != x) return false;
    return true;
  }
};

struct Planes {
  Guarded hdr, dot, clock, votes, nkeys, route, targets, lengths;
  fx_table_group_synth_planes c;
  Planes(uint32_t S, uint32_t steps, uint32_t vmax, size_t twords, uint32_t fill)
      : hdr(fx_plane_words(S, steps), fill), dot(fx_plane_words(S, steps), fill), clock(fx_plane_words(S, steps), fill),
        votes(fx_plane_words(S, steps) * 3 * vmax, fill), nkeys(fx_plane_words(S, steps), fill),
        route(fx_plane_words(S, steps), fill), targets(twords, fill), lengths(S, fill) {
    c = fx_table_group_synth_planes{hdr.data(),   dot.data(),     clock.data(),  votes.data(),
                                    nkeys.data(), route.data(), targets.data(), lengths.data()};
  }
  bool guards() const {
    return hdr.guards() && dot.guards() && clock.guards() && votes.guards() && nkeys.guards() && route.guards() &&
           targets.guards() && lengths.guards();
  }
  bool all(uint32_t x) const {
    return hdr.all(x) && dot.all(x) && clock.all(x) && votes.all(x) && nkeys.all(x) && route.all(x) && targets.all(x) &&
           lengths.all(x);
  }
};

struct Geom {
  uint32_t groups, shards, smax, n, fq, keys, kmax, cmds, window, lag, msg_lag, c0, c1, block;
  uint64_t seed;  // 0: the seed and the group_base of tests/table_group_synth_shapes.py
  uint32_t base;
};

fx_table_group_synth_params params(const Geom& g) {
  fx_table_group_synth_params p{};
  p.seed = g.seed ? g.seed : 20250312;
  p.groups = g.groups;
  p.group_base = g.seed ? g.base : 1000;
  p.shards = g.shards;
  p.smax = g.smax;
  p.n = g.n;
  p.fast_quorum = g.fq;
  p.keys = g.keys;
  p.cmds = g.cmds;
  p.kmax = g.kmax;
  p.window = g.window;
  p.lag = g.lag;
  p.msg_lag = g.msg_lag;
  p.num_conflicts = 2;
  p.conflict_pct[0] = g.c0;
  p.conflict_pct[1] = g.c1;
  p.conflict_block = g.block;
  return p;
}

void run(const Geom& geom) {
  const fx_table_group_synth_params p = params(geom);
  const uint32_t S = p.groups * p.shards;
  const uint32_t FILL = 0xA5A5A5A5u;
  uint32_t bound = 0, bound_out = 0, vmax = 0, longest = 0, steps_out = 0;
  uint64_t bound_words = 0, words = 0;
  EXPECT(fx_table_group_synth_shape(&p, &bound, &bound_out, &vmax, &bound_words) == FX_OK, "shape");
  Guarded len(S, FILL);
  EXPECT(fx_table_group_synth_count_host(&p, len.data(), &longest, &steps_out, &words) == FX_OK, "count");
  EXPECT(len.guards(), "count wrote outside the lengths");
  if (geom.seed) EXPECT(longest > p.cmds * p.n, "longest %u: no key with n + 1 events", longest);
  EXPECT(longest <= bound && steps_out <= bound_out && steps_out >= longest && vmax == p.fast_quorum &&
             words <= bound_words * p.groups,
         "longest %u bound %u steps_out %u bound %u words %llu", longest, bound, steps_out, bound_out,
         (unsigned long long)words);
  // one row or one targets word short: refused, nothing written
  if (longest > 0) {
    Planes small(S, longest - 1, vmax, words, FILL);
    EXPECT(fx_table_group_synth_generate_host(&p, &small.c, longest - 1, (uint32_t)words) == FX_ERR_CAPACITY, "rows");
    EXPECT(small.all(FILL) && small.guards(), "buffers written by a refused call");
  }
  if (words > 0) {
    Planes small(S, longest, vmax, words - 1, FILL);
    EXPECT(fx_table_group_synth_generate_host(&p, &small.c, longest, (uint32_t)words - 1) == FX_ERR_CAPACITY, "words");
    EXPECT(small.all(FILL) && small.guards(), "buffers written by a refused call");
  }
  // the exact fit and a fit with spare rows
  for (uint32_t steps : {longest ? longest : 1u, longest + 3}) {
    Planes pl(S, steps, vmax, words, FILL);
    EXPECT(fx_table_group_synth_generate_host(&p, &pl.c, steps, (uint32_t)words) == FX_OK, "generate, %u steps", steps);
    EXPECT(pl.guards(), "a guard word was written, %u steps", steps);
    const size_t pw = fx_plane_words(S, steps);
    const uint32_t spad = (S + 63u) / 64u * 64u, rows = (steps + 3u) / 4u * 4u;
    std::vector<uint8_t> used(words, 0);
    for (uint32_t s = 0; s < spad; ++s) {
      const uint32_t L = s < S ? pl.lengths[s] : 0;
      if (s < S) EXPECT(L == len[s], "stream %u: %u events, counted %u", s, L, len[s]);
      for (uint32_t r = 0; r < rows; ++r) {
        const size_t at = fx_index(r, s, steps);
        if (r < L) {
          const uint32_t nv = FX_TABLE_HDR_NVOTES(pl.hdr[at]);
          EXPECT(nv >= 1 && nv <= vmax && pl.votes[at] >= 1 && pl.votes[at] <= p.n && pl.votes[pw + at] >= 1 &&
                     pl.votes[pw + at] <= pl.votes[2 * pw + at] && FX_TABLE_HDR_KEY(pl.hdr[at]) < p.keys,
                 "stream %u row %u: malformed event", s, r);
          const bool attached = FX_TABLE_HDR_KIND(pl.hdr[at]) == FX_TABLE_ATTACHED;
          const uint32_t w = pl.nkeys[at], i = pl.route[at];
          if (!attached || FX_TABLE_PS_WORD_SHARDS(w) == 1) {
            EXPECT(i == FX_TABLE_ROUTE_NONE && (attached || w == 0), "stream %u row %u: route %u", s, r, i);
            continue;
          }
          EXPECT(FX_TABLE_PS_WORD_SHARDS(w) <= p.shards && FX_TABLE_PS_WORD_NKEYS(w) >= 1, "stream %u row %u", s, r);
          if (!(i < words && i + 1ull + pl.targets[i] <= words)) {
            EXPECT(false, "stream %u row %u: list %u outside targets", s, r, i);
            continue;
          }
          uint32_t others = 0, last = 0xFFFFFFFFu;
          for (uint32_t k = 0; k <= pl.targets[i]; ++k) used[i + k] = 1;
          for (uint32_t k = 1; k <= pl.targets[i]; ++k) {
            const uint32_t t = pl.targets[i + k], shard = t >> 24 & 7u;
            EXPECT(shard < p.shards && shard != s % p.shards && (t & 0xFFFFFFu) < p.keys && t >> 27 <= p.msg_lag,
                   "stream %u row %u: target %08x", s, r, t);
            others += shard != last;
            last = shard;
          }
          EXPECT(others == FX_TABLE_PS_WORD_SHARDS(w) - 1, "stream %u row %u: %u other shards", s, r, others);
        } else {
          bool zero = pl.hdr[at] == 0 && pl.dot[at] == 0 && pl.clock[at] == 0 && pl.nkeys[at] == 0 &&
                      pl.route[at] == FX_TABLE_ROUTE_NONE;
          for (uint32_t j = 0; j < 3 * vmax; ++j) zero = zero && pl.votes[j * pw + at] == 0;
          EXPECT(zero, "stream %u row %u past the length %u is not zero", s, r, L);
        }
      }
    }
    size_t unused = 0;
    for (uint8_t u : used) unused += !u;
    EXPECT(unused == 0, "%zu words of targets belong to no list", unused);
  }
}

}  // namespace

int main() {
  // (groups, shards, smax, n, fq, keys, kmax, cmds, window, lag, msg_lag, conflict rates, conflict_block):
  // tests/table_group_synth_shapes.py GEOMS, in its order (a copy: a geometry changed there is changed here)
  const Geom geoms[] = {
      {1, 2, 2, 3, 2, 16, 2, 40, 4, 6, 3, 2, 2, 0},     {65, 3, 3, 5, 3, 16, 2, 20, 4, 6, 3, 2, 50, 32},
      {3, 1, 1, 5, 3, 16, 2, 40, 4, 6, 0, 0, 0, 0},     {2, 3, 3, 3, 2, 1, 3, 40, 0, 0, 0, 2, 2, 0},
      {2, 8, 8, 3, 2, 2, 2, 30, 9, 3, 0, 2, 2, 0},      {2, 8, 8, 3, 2, 2, 2, 30, 9, 9, 31, 2, 2, 0},
      {2, 4, 2, 7, 4, 8, 2, 40, 4, 6, 3, 100, 100, 0},  {2, 2, 2, 5, 3, 16, 2, 40, 4, 6, 3, 100, 100, 0},
      {3, 3, 3, 5, 3, 33, 3, 40, 4, 6, 3, 2, 2, 0},     {2, 2, 2, 5, 3, 16, 2, 40, 50, 80, 3, 2, 2, 0},
      {3, 2, 2, 5, 3, 16, 2, 0, 4, 6, 3, 2, 2, 0},      {3, 3, 3, 5, 5, 16, 2, 1, 4, 6, 3, 2, 2, 0},
      {130, 2, 2, 5, 3, 64, 8, 10, 4, 6, 3, 2, 50, 0},  // the threads of the host twin, eight keys per shard
      // a key with n + 1 events (every process below a commit clock that comes from the other shard):
      // tests/test_table_group_synth_cpu.py ALL_BELOW
      {1, 2, 2, 3, 2, 16, 1, 3, 0, 0, 3, 0, 0, 0, 7, 1774},
      {1, 2, 2, 3, 2, 16, 1, 6, 0, 0, 3, 0, 0, 0, 7, 20146},
  };
  for (const Geom& g : geoms) run(g);
  // refused arguments leave the buffers alone
  {
    const Geom ok{1, 2, 2, 5, 3, 16, 2, 10, 4, 6, 3, 2, 2, 0};
    Geom bad[9] = {ok, ok, ok, ok, ok, ok, ok, ok, ok};
    bad[0].n = 17;
    bad[1].fq = 6;
    bad[2].shards = 0;
    bad[3].shards = FX_TABLE_MAX_CMD_SHARDS + 1u;
    bad[4].smax = 0;
    bad[5].smax = FX_TABLE_MAX_CMD_SHARDS + 1u;
    bad[6].msg_lag = FX_TABLE_GROUP_MAX_DELAY + 1u;
    bad[7].keys = 0;
    bad[8].c1 = 101;
    for (const Geom& g : bad) {
      const fx_table_group_synth_params p = params(g);
      Planes pl(2, 64, 5, 500, 0x5A5A5A5Au);
      EXPECT(fx_table_group_synth_generate_host(&p, &pl.c, 64, 500) == FX_ERR_INVALID_ARG, "bad arguments accepted");
      EXPECT(pl.all(0x5A5A5A5Au) && pl.guards(), "buffers written by a refused call");
      EXPECT(fx_table_group_synth_shape(&p, nullptr, nullptr, nullptr, nullptr) == FX_ERR_INVALID_ARG, "shape");
    }
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("table_group_synth_host_check: ok\n");
  return 0;
}
