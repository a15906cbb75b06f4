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
// The steps of a command -- ts_pick_keys, ts_pick_quorum, ts_propose,
// ts_emit_attached, ts_detach -- are stated once, here, over one set of clocks
// [key][process], one set of slot counters and one target stream; ts_walk
// composes them for a stream and tg_walk (fx_table_group_synth.h) per shard of
// a group.  A walk runs twice: the counting pass adds every event to its
// slot's counter; after an exclusive prefix over the slots the counters are
// row cursors and the emitting pass, walking the same draws, stores every
// event at its slot's cursor.  Events of a slot are created in the order they
// are stored, so no sort is needed.  The same function runs per lane in
// table_synth.hip and per stream in table_synth_host.cpp.
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

// the limits the stream and the group parameters share
template <class Params>
inline bool ts_common_ok(const Params& p) {
  if (p.n < 1 || p.n > 16 || p.fast_quorum < 1 || p.fast_quorum > p.n || p.kmax < 1 ||
      p.kmax > FX_TABLE_MAX_CMD_KEYS || p.keys < 1 || p.keys > FX_TABLE_SYNTH_MAX_KEYS || p.cmds > FX_SEQ_MASK ||
      p.window > FX_SEQ_MASK || p.lag > FX_SEQ_MASK || p.num_conflicts > 8)
    return false;
  for (uint32_t i = 0; i < (p.num_conflicts ? p.num_conflicts : 1u); ++i)
    if (p.conflict_pct[i] > 100) return false;
  return true;
}

inline int ts_check(const fx_table_synth_params* p) {
  if (!p || !ts_common_ok(*p)) return FX_ERR_INVALID_ARG;
  if ((uint64_t)p->stream_base + p->streams > (1ull << 32)) return FX_ERR_INVALID_ARG;
  const uint64_t kcap = p->kmax < p->keys ? p->kmax : p->keys;
  if ((uint64_t)p->cmds * kcap * p->n >= (1ull << 32)) return FX_ERR_INVALID_ARG;
  return FX_OK;
}

// words of per-stream state: the clocks [key][process], then the command
// counts of the coordinators
FX_HD uint32_t ts_state_words(const fx_table_synth_params& p) { return (p.keys + 1u) * p.n; }
// delivery slots of a stream (of either kind of parameters)
template <class Params>
FX_HD uint32_t ts_slots(const Params& p) {
  return p.cmds + (p.window > p.lag ? p.window : p.lag) + 1u;
}

struct TsStream {
  uint64_t seed, g;  // g: the global stream (the global group)
  uint32_t n, fq, keys, cmds, kcap, window, lag, conflict;
};

// what global stream (group) g takes from either kind of parameters
template <class Params>
FX_HD TsStream ts_model(const Params& p, uint64_t g) {
  TsStream ts;
  ts.seed = p.seed;
  ts.g = g;
  ts.n = p.n;
  ts.fq = p.fast_quorum;
  ts.keys = p.keys;
  ts.cmds = p.cmds;
  ts.kcap = p.kmax < p.keys ? p.kmax : p.keys;
  ts.window = p.window;
  ts.lag = p.lag;
  const uint32_t nc = p.num_conflicts ? p.num_conflicts : 1;
  const uint64_t ci = p.conflict_block ? (g / p.conflict_block) % nc : g % nc;
  ts.conflict = p.conflict_pct[ci];
  return ts;
}

FX_HD TsStream ts_stream(const fx_table_synth_params& p, uint32_t local) {
  return ts_model(p, (uint64_t)p.stream_base + local);
}

// words i * stride of an array: a stream's column of a [word][stream] table
struct TsWords {
  uint32_t* base;
  size_t stride;
  FX_HD uint32_t& operator[](size_t i) const { return base[i * stride]; }
  FX_HD TsWords from(size_t i) const { return TsWords{base + i * stride, stride}; }
};

// where the emitting pass stores: `stream` is the stream of ts_walk, shard 0
// of the group of tg_walk
struct TsOut {
  uint32_t *hdr, *dot, *clock, *votes, *nkeys;
  size_t plane;
  uint32_t steps, stream;
};

// What a generate call stores before its walks: 0 in every word of the planes
// (rows no stream reaches, the pad streams of the last tile), no route.  nkeys
// and route may be null.  set(p, byte, bytes): memset on the host, its
// asynchronous counterpart on the device; false stops.
template <class Set>
inline bool ts_clear_planes(Set set, const TsOut& o, uint32_t fast_quorum, uint32_t* route) {
  const size_t bytes = o.plane * 4;
  return set(o.hdr, 0, bytes) && set(o.dot, 0, bytes) && set(o.clock, 0, bytes) &&
         set(o.votes, 0, bytes * 3 * fast_quorum) && (!o.nkeys || set(o.nkeys, 0, bytes)) &&
         (!route || set(route, 0xFF, bytes));
}

// the draws of one (seed, stream or group, a)
struct TsDraw {
  uint64_t seed, g, a;
  FX_HD uint32_t operator()(uint64_t purpose, uint32_t m) const {
    return (uint32_t)(synth_rand(seed, g, a, purpose) % m);
  }
};

// the r-th smallest id below `count` whose bit in `taken` is clear
FX_HD uint32_t ts_pick_free(uint32_t taken, uint32_t r, uint32_t count) {
  uint32_t q = 0;
  for (; q < count; ++q) {
    if (taken >> q & 1u) continue;
    if (r == 0) break;
    --r;
  }
  return q;
}

// the K keys of a command, ascending; ck[K ..] = 0xFFFFFFFF
FX_HD void ts_pick_keys(const TsDraw& draw, uint32_t keys, uint32_t conflict, uint32_t K,
                        uint32_t (&ck)[FX_TABLE_MAX_CMD_KEYS]) {
  constexpr uint32_t KMAX = FX_TABLE_MAX_CMD_KEYS;
  ck[0] = (keys == 1 || draw(TS_CONFLICT, 100u) < conflict) ? 0u : 1u + draw(TS_FIRST, keys - 1u);
#pragma unroll
  for (uint32_t j = 1; j < KMAX; ++j) {
    ck[j] = 0xFFFFFFFFu;
    if (j < K) {
      uint32_t x = draw(TS_KEY + j, keys - j);
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
}

// the quorum of coordinator p (processes 0 .. n-1 in here), 4 bits per member
// in pick order
FX_HD uint64_t ts_pick_quorum(const TsDraw& draw, uint32_t p, uint32_t n, uint32_t fq) {
  uint64_t members = p;
  uint32_t chosen = 1u << p;
  for (uint32_t j = 1; j < fq; ++j) {
    const uint32_t q = ts_pick_free(chosen, draw(TS_QUORUM + j, n - j), n);
    chosen |= 1u << q;
    members |= (uint64_t)q << (4u * j);
  }
  return members;
}

// The proposals over clocks [key][process], member by member; the votes go
// straight to rows row0 .. row0 + K-1 of `stream`.  Returns the highest.
template <bool EMIT>
FX_HD uint32_t ts_propose(const TsWords clocks, uint32_t n, uint32_t fq, uint64_t members, uint32_t K,
                          const uint32_t (&ck)[FX_TABLE_MAX_CMD_KEYS], uint32_t row0, const TsOut& o,
                          uint32_t stream) {
  constexpr uint32_t KMAX = FX_TABLE_MAX_CMD_KEYS;
  uint32_t first = 0, highest = 0;
  for (uint32_t m = 0; m < fq; ++m) {
    const uint32_t q = (uint32_t)(members >> (4u * m)) & 15u;
    uint32_t top = 0;
#pragma unroll
    for (uint32_t k = 0; k < KMAX; ++k)
      if (k < K) {
        const uint32_t c = clocks[(size_t)ck[k] * n + q];
        top = c > top ? c : top;
      }
    const uint32_t prop = m == 0 || top + 1u > first ? top + 1u : first;
    if (m == 0) first = prop;
    highest = prop > highest ? prop : highest;
#pragma unroll
    for (uint32_t k = 0; k < KMAX; ++k)
      if (k < K) {
        const size_t w = (size_t)ck[k] * n + q;
        if (EMIT && row0 + k < o.steps) {
          uint32_t* v = o.votes + (size_t)(3u * m) * o.plane + fx_index(row0 + k, stream, o.steps);
          v[0] = q + 1u;
          v[o.plane] = clocks[w] + 1u;
          v[2 * o.plane] = prop;
        }
        clocks[w] = prop;
      }
  }
  return highest;
}

// The rest of the K attached events, once the commit clock is known.  word:
// what the nkeys plane (if any) takes; route (optional): the plane that takes
// `list`.
template <bool EMIT>
FX_HD void ts_emit_attached(const TsOut& o, uint32_t stream, uint32_t row0, uint32_t K,
                            const uint32_t (&ck)[FX_TABLE_MAX_CMD_KEYS], uint32_t fq, uint32_t dot, uint32_t commit,
                            uint32_t word, uint32_t* route, uint32_t list) {
  constexpr uint32_t KMAX = FX_TABLE_MAX_CMD_KEYS;
  if (!EMIT) return;
#pragma unroll
  for (uint32_t k = 0; k < KMAX; ++k)
    if (k < K && row0 + k < o.steps) {
      const size_t at = fx_index(row0 + k, stream, o.steps);
      o.hdr[at] = FX_TABLE_HDR(FX_TABLE_ATTACHED, fq, ck[k]);
      o.dot[at] = dot;
      o.clock[at] = commit;
      if (o.nkeys) o.nkeys[at] = word;
      if (route) route[at] = list;
    }
}

// Detached votes of the command's key index k (key id `key`): every process
// below the commit clock, each in a slot of its own from command i on.  The
// walks call it per key under #pragma unroll: with the loop over ck[] in here
// the on-chip counting kernel of the streams takes 74 VGPRs instead of 62 and
// loses a wavefront of occupancy.
template <bool EMIT>
FX_HD void ts_detach(const TsDraw& draw, const TsWords clocks, const TsWords slots, uint32_t n, uint32_t i,
                     uint32_t lag, uint32_t k, uint32_t key, uint32_t commit, const TsOut& o, uint32_t stream) {
  for (uint32_t q = 0; q < n; ++q) {
    const size_t w = (size_t)key * n + q;
    const uint32_t own = clocks[w];
    if (own >= commit) continue;
    clocks[w] = commit;
    const uint32_t ds = i + draw(TS_LAG + 16u * k + q, lag + 1u);
    const uint32_t row = slots[ds];
    slots[ds] = row + 1u;
    if (EMIT && row < o.steps) {
      const size_t at = fx_index(row, stream, o.steps);
      o.hdr[at] = FX_TABLE_HDR(FX_TABLE_DETACHED, 1u, key);
      o.votes[at] = q + 1u;
      o.votes[o.plane + at] = own + 1u;
      o.votes[2 * o.plane + at] = commit;
    }
  }
}

// state: ts_state_words words, zeroed here.  slots: ts_slots words; EMIT
// false: zero on entry, counts on return; EMIT true: every slot's first row on
// entry.  A row at or past o.steps is never stored.
template <bool EMIT>
FX_HD void ts_walk(const TsStream& ts, const TsWords state, const TsWords slots, const TsOut& o) {
  const uint32_t n = ts.n, seqs = ts.keys * n;
  for (uint32_t w = 0; w < seqs + n; ++w) state[w] = 0;
  for (uint32_t i = 0; i < ts.cmds; ++i) {
    const TsDraw draw{ts.seed, ts.g, i};
    const uint32_t K = 1u + draw(TS_COUNT, ts.kcap);
    uint32_t ck[FX_TABLE_MAX_CMD_KEYS];
    ts_pick_keys(draw, ts.keys, ts.conflict, K, ck);
    const uint32_t p = draw(TS_COORD, n);
    const uint64_t members = ts_pick_quorum(draw, p, n, ts.fq);
    const uint32_t seq = state[seqs + p] + 1u;
    state[seqs + p] = seq;
    const uint32_t slot = i + draw(TS_WINDOW, ts.window + 1u);
    const uint32_t row0 = slots[slot];
    slots[slot] = row0 + K;
    const uint32_t commit = ts_propose<EMIT>(state, n, ts.fq, members, K, ck, row0, o, o.stream);
    ts_emit_attached<EMIT>(o, o.stream, row0, K, ck, ts.fq, FX_PACK_DOT(p + 1u, seq), commit, K, nullptr, 0u);
#pragma unroll
    for (uint32_t k = 0; k < FX_TABLE_MAX_CMD_KEYS; ++k)
      if (k < K) ts_detach<EMIT>(draw, state, slots, n, i, ts.lag, k, ck[k], commit, o, o.stream);
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
