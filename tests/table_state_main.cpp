// The state layout of a resumable table-executor stream
// (fantoch_amd/csrc/table_state.h) on the host: every index the kernels of
// fx_table_advance use is marked in an array of exactly one stream's stride,
// so an index beyond it is out of bounds under the sanitizers and one used
// twice is reported here.
//
//   table_state_main KIND KEYS
//
// Prints `stride image_at words-marked` (in 32-bit words) and exits 0, or 3
// when two indices meet or words of the stride are left over.
// tests/test_table_state_cpu.py compares the stride with fx_table_session_bytes.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "table_state.h"

using namespace fx::table;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const uint32_t kind = (uint32_t)strtoul(argv[1], nullptr, 10), keys = (uint32_t)strtoul(argv[2], nullptr, 10);
  if (kind > FX_TABLE_KIND_PS || keys < 1) return 2;
  const size_t stride = ts_stride(kind, keys), at = ts_image_at(kind, keys);
  std::vector<unsigned char> used(stride, 0);
  size_t marked = 0;
  bool twice = false;
  auto mark = [&](size_t i) {
    if (used[i]++) twice = true;
    ++marked;
  };
  // the tables: frontier rows, window rows (16 voter columns each), then the buffered entries of _ps
  for (size_t j = 0; j < (size_t)keys * (1u + TS_WB); ++j)
    for (uint32_t v = 0; v < TS_NV; ++v) mark(j * TS_NV + v);
  if (kind == FX_TABLE_KIND_PS)
    for (uint32_t e = 0; e < 3u * FX_TABLE_PS_HBM_BUFFERED; ++e) mark(ts_votes_words(keys) + e);
  if (marked != ts_tables_words(kind, keys)) return 3;
  // the image: the header row (all 64 words of it belong to the header), the register planes, _mk's entries
  for (uint32_t w = 0; w < 64u; ++w) mark(at + ts_hdr(w));
  if (TS_H_WORDS > 64u) return 3;
  for (uint32_t p = 0; p < ts_planes(kind); ++p)
    for (uint32_t i = 0; i < TS_R; ++i)
      for (uint32_t l = 0; l < 64u; ++l) mark(at + ts_reg(p, i, l));
  if (kind == FX_TABLE_KIND_MK)
    for (uint32_t j = 0; j < 3u; ++j)
      for (uint32_t l = 0; l < 64u; ++l) mark(at + ts_buf(j, l));
  printf("%zu %zu %zu\n", stride, at, marked);
  return twice || marked != stride ? 3 : 0;
}
