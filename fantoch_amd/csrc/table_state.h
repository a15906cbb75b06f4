// table_state.h — where a resumable table-executor stream (fx_table_advance,
// table_exec.hip) keeps what it carries from one call to the next: the index
// arithmetic of one stream's part of `state`, in 32-bit words.  Plain integer
// code, so a host compiler takes it too (tests/table_state_main.cpp checks
// that no two indices meet and that all lie inside fx_table_session_bytes).
//
//   [0, ts_tables_words)   the votes tables, as at FX_TABLE_TIER_HBM (frontiers,
//                          then the ring windows), and for FX_TABLE_KIND_PS the
//                          buffered (key, dot, count) table behind them
//   [ts_image_at, stride)  the image of the wavefront's registers, rows of 64
//                          words, word l of a row owned by lane l (lane-major:
//                          a row is one coalesced load or store):
//     row 0                the header words TS_H_*
//     ts_reg(p, i, l)      register row i (< TS_R) of plane p (TS_P_*) on lane l
//     ts_buf(j, l)         FX_TABLE_KIND_MK: the lane's buffered (key, dot,
//                          count) entry, j = 0..2
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fantoch_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FX_TS_FN __host__ __device__ constexpr inline
#else
#define FX_TS_FN constexpr inline
#endif

namespace fx {
namespace table {

constexpr uint32_t TS_NV = 16;                           // voter columns of a votes table
constexpr uint32_t TS_WB = FX_TABLE_HBM_WINDOW / 32u;    // window words per (key, voter)
constexpr uint32_t TS_R = FX_TABLE_HBM_PENDING / 64u;    // register rows per plane

// header words (row 0 of the image).  The first seven are the session
// contract: a call whose arguments differ stops the stream.
enum : uint32_t {
  TS_H_STEPS = 0, TS_H_N, TS_H_KEYS, TS_H_VMAX, TS_H_THR, TS_H_KIND, TS_H_AT_COMMIT,
  TS_H_DONE,   // rows handled so far: the next call starts here
  TS_H_NEXEC, TS_H_ERR,
  TS_H_QSEQ, TS_H_MB, TS_H_MT,  // _mk, _ps: the FIFO counter, to_executors = messages [mb, mt)
  TS_H_NBUF, TS_H_BHI,          // buffered pairs alive; _ps: rows of the buffered table ever used
  TS_H_WORDS
};
// register planes: pending ops (key, clock, dot, arrival); _mk, _ps: the op's
// meta word and the to_executors ring (key, dot); _ps: missing | shards << 8
enum : uint32_t { TS_P_KEY = 0, TS_P_CLOCK, TS_P_DOT, TS_P_ARRIVAL, TS_P_META, TS_P_RING_KEY, TS_P_RING_DOT, TS_P_SHARDS };

FX_TS_FN uint32_t ts_planes(uint32_t kind) {
  return kind == FX_TABLE_KIND_SINGLE ? 4u : kind == FX_TABLE_KIND_MK ? 7u : 8u;
}
FX_TS_FN size_t ts_votes_words(uint32_t keys) { return (size_t)keys * TS_NV * (1u + TS_WB); }
FX_TS_FN size_t ts_tables_words(uint32_t kind, uint32_t keys) {
  return ts_votes_words(keys) + (kind == FX_TABLE_KIND_PS ? 3u * FX_TABLE_PS_HBM_BUFFERED : 0u);
}
FX_TS_FN size_t ts_image_at(uint32_t kind, uint32_t keys) { return ts_tables_words(kind, keys); }
FX_TS_FN uint32_t ts_image_words(uint32_t kind) {
  return 64u * (1u + ts_planes(kind) * TS_R + (kind == FX_TABLE_KIND_MK ? 3u : 0u));
}
FX_TS_FN size_t ts_stride(uint32_t kind, uint32_t keys) { return ts_image_at(kind, keys) + ts_image_words(kind); }
// relative to ts_image_at
FX_TS_FN uint32_t ts_hdr(uint32_t word) { return word; }
FX_TS_FN uint32_t ts_reg(uint32_t plane, uint32_t row, uint32_t lane) { return 64u * (1u + plane * TS_R + row) + lane; }
FX_TS_FN uint32_t ts_buf(uint32_t j, uint32_t lane) { return 64u * (1u + 7u * TS_R + j) + lane; }

}  // namespace table
}  // namespace fx
