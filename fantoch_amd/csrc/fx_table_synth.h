// fx_table_synth.h — seeded synthetic Tempo vote streams (host + device).
//
// The table executor's counterpart of fx_synth.h: stands in for the
// TableExecutionInfo values Tempo's clock-and-vote side hands its executor
// (fantoch_ps/src/protocol/tempo.rs:614-636) until a Tempo simulator exists.
// Per stream, n processes keep a clock per key (SequentialKeyClocks,
// fantoch_ps/src/protocol/common/table/clocks/keys/sequential.rs:38-114).
// Command i = 0 .. cmds-1 of global stream g; every draw is
// synth_rand(seed, g, i, purpose), a range is draw % m (canonical C6):
//   * key count   K = 1 + draw(TS_COUNT) % min(kmax, keys)
//   * first key   0 if keys == 1 or draw(TS_CONFLICT) % 100 < conflict,
//                 else 1 + draw(TS_FIRST) % (keys - 1)
//   * further key j = 1 .. K-1: the (draw(TS_KEY + j) % (keys - j))-th smallest
//                 key id not yet chosen; the keys are taken ascending (C11)
//   * coordinator p = 1 + draw(TS_COORD) % n
//   * quorum      member j = 1 .. fast_quorum-1: the
//                 (draw(TS_QUORUM + j) % (n - j))-th smallest process not yet
//                 chosen (p is); votes list p, then the members as picked
//   * clocks      p proposes max over the keys of its clock + 1, a member the
//                 higher of that and its own highest + 1 (proposal,
//                 sequential.rs:38-57); each votes own(x) + 1 .. its proposal
//                 on every key x and moves there; commit = highest proposal;
//                 dot (p, seq), seq counted per coordinator from 1
//   * events      K attached (keys ascending, FX_TABLE_HDR(FX_TABLE_ATTACHED,
//                 fast_quorum, key), dot, commit, the key's votes, nkeys = K);
//                 then for keys ascending, processes ascending, every process
//                 below commit on the key: one detached event own + 1 ..
//                 commit (detached, sequential.rs:59-70, 99-114)
//   * delivery    the attached events share slot i + draw(TS_WINDOW) %
//                 (window + 1); a detached event of key index k, process q has
//                 slot i + draw(TS_LAG + 16 k + q - 1) % (lag + 1); a stream is
//                 its events by (slot, creation order).
// A command makes at most K n events (the member with the highest proposal is
// at the commit clock on every key), and an event carries at most fast_quorum
// vote ranges.
//
// ts_walk is the one statement of the model: the counting pass adds every
// event to its slot's counter; after an exclusive prefix over the slots the
// counters are row cursors and the emitting pass, walking the same draws,
// stores every event at its slot's cursor.  Events of a slot are created in
// the order they are stored, so no sort is needed.  The same function runs per
// lane in table_synth.hip and per stream in table_synth_host.cpp.
#pragma once
#include <stdint.h>

#include "fx_synth.h"

namespace fx {

// purposes of the draws (the last argument of synth_rand, below 256)
enum : uint64_t {
  TS_COUNT = 32,     // key count
  TS_CONFLICT = 33,  // first key: the conflict key?
  TS_FIRST = 34,     // first key otherwise
  TS_COORD = 35,     // coordinator
  TS_WINDOW = 36,    // slot of the attached events
  TS_KEY = 40,       // + j: further key j = 1 .. 7
  TS_QUORUM = 48,    // + j: quorum member j = 1 .. 15
  TS_LAG = 128       // + 16 * key index + process - 1: slot of a detached event
};

inline int ts_check(const fx_table_synth_params* p) {
  if (!p || p->n < 1 || p->n > 16 || p->fast_quorum < 1 || p->fast_quorum > p->n || p->kmax < 1 ||
      p->kmax > FX_TABLE_MAX_CMD_KEYS || p->keys < 1 || p->keys > FX_TABLE_SYNTH_MAX_KEYS || p->cmds > FX_SEQ_MASK ||
      p->window > FX_SEQ_MASK || p->lag > FX_SEQ_MASK || p->num_conflicts > 8)
    return FX_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < (p->num_conflicts ? p->num_conflicts : 1u); ++i)
    if (p->conflict_pct[i] > 100) return FX_ERR_INVALID_ARG;
  if ((uint64_t)p->stream_base + p->streams > (1ull << 32)) return FX_ERR_INVALID_ARG;
  const uint64_t kcap = p->kmax < p->keys ? p->kmax : p->keys;
  if ((uint64_t)p->cmds * kcap * p->n >= (1ull << 32)) return FX_ERR_INVALID_ARG;
  return FX_OK;
}

// words of per-stream state: the clocks [key][process], then the command
// counts of the coordinators
FX_HD uint32_t ts_state_words(const fx_table_synth_params& p) { return (p.keys + 1u) * p.n; }
// delivery slots of a stream
FX_HD uint32_t ts_slots(const fx_table_synth_params& p) {
  return p.cmds + (p.window > p.lag ? p.window : p.lag) + 1u;
}

struct TsStream {
  uint64_t seed, g;  // g: the global stream
  uint32_t n, fq, keys, cmds, kcap, window, lag, conflict;
};

FX_HD TsStream ts_stream(const fx_table_synth_params& p, uint32_t local) {
  TsStream ts;
  ts.seed = p.seed;
  ts.g = (uint64_t)p.stream_base + local;
  ts.n = p.n;
  ts.fq = p.fast_quorum;
  ts.keys = p.keys;
  ts.cmds = p.cmds;
  ts.kcap = p.kmax < p.keys ? p.kmax : p.keys;
  ts.window = p.window;
  ts.lag = p.lag;
  const uint32_t nc = p.num_conflicts ? p.num_conflicts : 1;
  const uint64_t ci = p.conflict_block ? (ts.g / p.conflict_block) % nc : ts.g % nc;
  ts.conflict = p.conflict_pct[ci];
  return ts;
}

// words i * stride of an array: a stream's column of a [word][stream] table
struct TsWords {
  uint32_t* base;
  size_t stride;
  FX_HD uint32_t& operator[](size_t i) const { return base[i * stride]; }
};

// where the emitting pass stores stream `stream`
struct TsOut {
  uint32_t *hdr, *dot, *clock, *votes, *nkeys;
  size_t plane;
  uint32_t steps, stream;
};

// state: ts_state_words words, zeroed here.  slots: ts_slots words; EMIT
// false: zero on entry, counts on return; EMIT true: every slot's first row on
// entry.  A row at or past o.steps is never stored.
template <bool EMIT>
FX_HD void ts_walk(const TsStream& ts, const TsWords state, const TsWords slots, const TsOut& o) {
  constexpr uint32_t KMAX = FX_TABLE_MAX_CMD_KEYS;
  const uint32_t n = ts.n, keys = ts.keys;
  const uint32_t seqs = keys * n;
  for (uint32_t w = 0; w < seqs + n; ++w) state[w] = 0;
  for (uint32_t i = 0; i < ts.cmds; ++i) {
    const uint32_t K = 1u + (uint32_t)(synth_rand(ts.seed, ts.g, i, TS_COUNT) % ts.kcap);
    uint32_t ck[KMAX];  // the command's keys, ascending
    ck[0] = (keys == 1 || (uint32_t)(synth_rand(ts.seed, ts.g, i, TS_CONFLICT) % 100u) < ts.conflict)
                ? 0u
                : 1u + (uint32_t)(synth_rand(ts.seed, ts.g, i, TS_FIRST) % (keys - 1u));
#pragma unroll
    for (uint32_t j = 1; j < KMAX; ++j) {
      ck[j] = 0xFFFFFFFFu;
      if (j < K) {
        uint32_t x = (uint32_t)(synth_rand(ts.seed, ts.g, i, TS_KEY + j) % (keys - j));
#pragma unroll
        for (uint32_t t = 0; t < j; ++t)
          if (ck[t] <= x) ++x;
        ck[j] = x;
#pragma unroll
        for (uint32_t t = j; t > 0; --t)
          if (ck[t - 1] > ck[t]) {
            const uint32_t y = ck[t];
            ck[t] = ck[t - 1];
            ck[t - 1] = y;
          }
      }
    }
    const uint32_t p = (uint32_t)(synth_rand(ts.seed, ts.g, i, TS_COORD) % n);  // processes 0 .. n-1 in here
    // the quorum, 4 bits per member in pick order
    uint64_t members = p;
    uint32_t chosen = 1u << p;
    for (uint32_t j = 1; j < ts.fq; ++j) {
      uint32_t r = (uint32_t)(synth_rand(ts.seed, ts.g, i, TS_QUORUM + j) % (n - j));
      uint32_t q = 0;
      for (; q < n; ++q) {
        if (chosen >> q & 1u) continue;
        if (r == 0) break;
        --r;
      }
      chosen |= 1u << q;
      members |= (uint64_t)q << (4u * j);
    }
    const uint32_t seq = state[seqs + p] + 1u;
    state[seqs + p] = seq;
    const uint32_t slot = i + (uint32_t)(synth_rand(ts.seed, ts.g, i, TS_WINDOW) % (ts.window + 1u));
    const uint32_t row0 = slots[slot];
    slots[slot] = row0 + K;
    // proposals, member by member; the votes go straight to the K rows
    uint32_t first = 0, commit = 0;
    for (uint32_t m = 0; m < ts.fq; ++m) {
      const uint32_t q = (uint32_t)(members >> (4u * m)) & 15u;
      uint32_t top = 0;
#pragma unroll
      for (uint32_t k = 0; k < KMAX; ++k)
        if (k < K) {
          const uint32_t c = state[(size_t)ck[k] * n + q];
          top = c > top ? c : top;
        }
      const uint32_t prop = m == 0 || top + 1u > first ? top + 1u : first;
      if (m == 0) first = prop;
      commit = prop > commit ? prop : commit;
#pragma unroll
      for (uint32_t k = 0; k < KMAX; ++k)
        if (k < K) {
          const size_t w = (size_t)ck[k] * n + q;
          if (EMIT && row0 + k < o.steps) {
            uint32_t* v = o.votes + (size_t)(3u * m) * o.plane + fx_index(row0 + k, o.stream, o.steps);
            v[0] = q + 1u;
            v[o.plane] = state[w] + 1u;
            v[2 * o.plane] = prop;
          }
          state[w] = prop;
        }
    }
    if (EMIT) {
#pragma unroll
      for (uint32_t k = 0; k < KMAX; ++k)
        if (k < K && row0 + k < o.steps) {
          const size_t at = fx_index(row0 + k, o.stream, o.steps);
          o.hdr[at] = FX_TABLE_HDR(FX_TABLE_ATTACHED, ts.fq, ck[k]);
          o.dot[at] = FX_PACK_DOT(p + 1u, seq);
          o.clock[at] = commit;
          if (o.nkeys) o.nkeys[at] = K;
        }
    }
    // detached votes: every process below the commit clock, per key
#pragma unroll
    for (uint32_t k = 0; k < KMAX; ++k)
      if (k < K)
        for (uint32_t q = 0; q < n; ++q) {
          const size_t w = (size_t)ck[k] * n + q;
          const uint32_t own = state[w];
          if (own >= commit) continue;
          state[w] = commit;
          const uint32_t ds = i + (uint32_t)(synth_rand(ts.seed, ts.g, i, TS_LAG + 16u * k + q) % (ts.lag + 1u));
          const uint32_t row = slots[ds];
          slots[ds] = row + 1u;
          if (EMIT && row < o.steps) {
            const size_t at = fx_index(row, o.stream, o.steps);
            o.hdr[at] = FX_TABLE_HDR(FX_TABLE_DETACHED, 1u, ck[k]);
            o.votes[at] = q + 1u;
            o.votes[o.plane + at] = own + 1u;
            o.votes[2 * o.plane + at] = commit;
          }
        }
  }
}

// counts -> first rows (exclusive prefix over the slots); returns the length
FX_HD uint32_t ts_prefix(const TsWords slots, uint32_t nslots) {
  uint32_t run = 0;
  for (uint32_t t = 0; t < nslots; ++t) {
    const uint32_t c = slots[t];
    slots[t] = run;
    run += c;
  }
  return run;
}

}  // namespace fx
