// The table executor's window arithmetic (fantoch_amd/csrc/table_window.h) on
// the host: one voter's column of one key, laid out as the HBM kernel lays it
// out (word i at column[i * 16 + lane]), driven by `start end` lines on stdin.
//
//   table_window_main FORM FRONTIER
//     FORM      word | word_aligned | ring | ring_unrolled (the two layouts of the ring form)
//     FRONTIER  where the voter's frontier starts, with nothing above it
//
// After each line: `status frontier votes-held-above-the-frontier`.
// tests/test_table_window_cpu.py builds this under the host sanitizers and
// compares every line with the restatement's EventSet.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "table_window.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const bool ring = !strcmp(argv[1], "ring"), unrolled = !strcmp(argv[1], "ring_unrolled");
  const bool aligned = !strcmp(argv[1], "word_aligned");
  if (!ring && !unrolled && !aligned && strcmp(argv[1], "word")) return 2;
  constexpr uint32_t NV = 16, WB = FX_TABLE_HBM_WINDOW / 32u, LANE = 5;
  // exactly the words of one key's windows: a word index beyond the ring is out of bounds
  std::vector<uint32_t> column((size_t)WB * NV, 0u);
  uint32_t f = (uint32_t)strtoul(argv[2], nullptr, 10), w = 0;
  unsigned long st, en;
  while (scanf("%lu %lu", &st, &en) == 2) {
    uint32_t status;
    if (ring) status = fx::table::add_range_ring<true>(f, column.data() + LANE, NV, (uint32_t)st, (uint32_t)en);
    else if (unrolled) status = fx::table::add_range_ring<false>(f, column.data() + LANE, NV, (uint32_t)st, (uint32_t)en);
    else if (aligned) status = fx::table::add_range_word<true>(f, w, (uint32_t)st, (uint32_t)en);
    else status = fx::table::add_range_word<false>(f, w, (uint32_t)st, (uint32_t)en);
    unsigned held = (unsigned)__builtin_popcount(w);
    for (size_t i = 0; i < column.size(); ++i) {
      if (i % NV != LANE && column[i]) return 3;  // another voter's column was written
      held += (unsigned)__builtin_popcount(column[i]);
    }
    printf("%u %u %u\n", status, f, held);
  }
  return 0;
}
