// table_window.h — add_range (fantoch_ps/src/executor/table/mod.rs:180) of
// one voter on one key, as the table executor's kernels run it on the voter's
// lane (table_exec.hip): the frontier (every vote 1..f seen) and the votes
// seen above it.  Plain integer code, so a host compiler takes it too
// (tests/table_window_main.cpp runs it against the restatement's EventSet).
//
// Both forms take a range with 1 <= st <= en (the caller checks that) and
// return 0, FX_ERR_VOTE_RANGE (no vote of the range is new) or FX_ERR_CAPACITY
// (a new vote lies beyond the window and the range leaves a gap below it).
// A failing call leaves the frontier and the window as they were.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fantoch_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FX_TW_FN __host__ __device__ __forceinline__
#else
#define FX_TW_FN inline
#endif
#if defined(__clang__)
#define FX_TW_NOUNROLL _Pragma("nounroll")
#else
#define FX_TW_NOUNROLL
#endif

namespace fx {
namespace table {

FX_TW_FN uint32_t low_mask(uint32_t cnt) { return cnt >= 32u ? ~0u : (1u << cnt) - 1u; }
FX_TW_FN uint32_t tw_ctz(uint32_t x) { return (uint32_t)__builtin_ctz(x); }

// ONCHIP: the window is one word relative to the frontier, bit i = vote
// f + 1 + i.  ALIGNED (the _mk and _ps kernels): a range that starts at the
// frontier moves it to `en` whatever its length (Tempo bumps a key's clock to
// the highest of a command's keys: such ranges are long); every vote of the
// window lies below.
template <bool ALIGNED>
FX_TW_FN uint32_t add_range_word(uint32_t& frontier, uint32_t& window, uint32_t st, uint32_t en) {
  // on copies, written back once: through the references the short branches
  // below stay branches; on values they become selects, as they were when
  // this text stood in the kernel
  uint32_t f = frontier, w = window, lf = 0;
  if (en <= f) {
    lf = FX_ERR_VOTE_RANGE;  // every vote of the range is at or below the frontier
  } else if (ALIGNED && en - f > FX_TABLE_ONCHIP_WINDOW && st <= f + 1u) {
    f = en;
    w = 0;
  } else if (en - f > FX_TABLE_ONCHIP_WINDOW) {
    lf = FX_ERR_CAPACITY;  // (the vote `en` lies beyond the window: it is new)
  } else {
    const uint32_t lo = st > f + 1u ? st : f + 1u;
    const uint32_t mask = low_mask(en - lo + 1u) << (lo - f - 1u);
    if (!(mask & ~w)) {
      lf = FX_ERR_VOTE_RANGE;
    } else {
      w |= mask;
      const uint32_t t = w == ~0u ? 32u : tw_ctz(~w);
      f += t;
      w = t >= 32u ? 0u : w >> t;
    }
  }
  frontier = f;
  window = w;
  return lf;
}

// HBM: a ring of FX_TABLE_HBM_WINDOW bits, vote v at bit v & 31 of word
// (v & (FX_TABLE_HBM_WINDOW - 1)) >> 5; word i at win[i * stride].  The votes
// f + 1 .. f + FX_TABLE_HBM_WINDOW have distinct bits and every bit of a vote
// at or below f is clear.  A range that starts at the frontier and ends beyond
// the window moves the frontier to `en` and clears the ring: every recorded
// vote lies at or below `en`.  COMPACT keeps that loop rolled: the HBM kernels
// are larger than the instruction cache and their step time follows the
// layout of this rare path -- measured (profiles/r10_table_edges_bench.json),
// the single-key and _mk kernels are faster with the rolled loop, the _ps
// kernel with the unrolled one.
template <bool COMPACT>
FX_TW_FN uint32_t add_range_ring(uint32_t& frontier, uint32_t* win, size_t stride, uint32_t st, uint32_t en) {
  constexpr uint32_t W = FX_TABLE_HBM_WINDOW;
  uint32_t f = frontier, lf = 0;
  if (en <= f) {
    lf = FX_ERR_VOTE_RANGE;  // every vote of the range is at or below the frontier
  } else if (__builtin_expect(en - f > W, 0)) {  // rare: kept small and out of the way of the ranges inside the window
    if (st <= f + 1u) {
      if (COMPACT) {
        FX_TW_NOUNROLL
        for (uint32_t i = 0; i < W / 32u; ++i) win[(size_t)i * stride] = 0;
      } else {
        for (uint32_t i = 0; i < W / 32u; ++i) win[(size_t)i * stride] = 0;
      }
      f = en;
    } else {
      lf = FX_ERR_CAPACITY;  // (the vote `en` lies beyond the window: it is new)
    }
  } else {
    uint32_t any = 0, v = st > f + 1u ? st : f + 1u;
    for (uint32_t rem = en - v + 1u; rem;) {
      const uint32_t bp = v & 31u, cnt = 32u - bp < rem ? 32u - bp : rem;
      const uint32_t mask = low_mask(cnt) << bp, i = (v & (W - 1u)) >> 5;
      const uint32_t ww = win[(size_t)i * stride];
      any |= mask & ~ww;
      win[(size_t)i * stride] = ww | mask;
      v += cnt;
      rem -= cnt;
    }
    if (!any) {
      lf = FX_ERR_VOTE_RANGE;
    } else {
      for (;;) {  // the frontier moves over the votes now contiguous with it
        const uint32_t nx = f + 1u, bp = nx & 31u, i = (nx & (W - 1u)) >> 5;
        const uint32_t ww = win[(size_t)i * stride], x = ~(ww >> bp);
        const uint32_t run = x ? tw_ctz(x) : 32u, t = run < 32u - bp ? run : 32u - bp;
        if (!t) break;
        win[(size_t)i * stride] = ww & ~(low_mask(t) << bp);
        f += t;
        if (t < 32u - bp) break;
      }
    }
  }
  frontier = f;
  return lf;
}

}  // namespace table
}  // namespace fx
