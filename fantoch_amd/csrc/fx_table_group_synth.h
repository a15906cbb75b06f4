// fx_table_group_synth.h — seeded closed-loop shard groups (host + device).
//
// The input of fx_table_run_groups, generated: what fx_table_synth.h is to
// fx_table_run_mk.  The model is tests/table_shapes_ps.synth_table_group's with
// every draw taken from the counter RNG.  Global group G has P shard
// executors, each with its own n processes and a clock per key
// (clocks[shard][key][process]).  Command i = 0 .. cmds-1 of the group; every
// draw is synth_rand(seed, G, a, purpose), a range is draw % m (canonical C6).
// Group level, a = i:
//   * shard count C = 1 + draw(TG_SHARDS) % min(smax, P)
//   * shard j = 0 .. C-1: the (draw(TG_SHARD + j) % (P - j))-th smallest shard
//                 not yet chosen; the shards are taken ascending
//   * coordinator p = 1 + draw(TG_COORD) % n, one for the whole command; dot
//                 (p, seq), seq counted per coordinator over the group from 1
// Per shard h of the set, a = i | (h + 1) << 32, with the purposes and the
// rules of fx_table_synth.h (TS_COORD is not drawn):
//   * keys        TS_COUNT, TS_CONFLICT, TS_FIRST, TS_KEY + j; the conflict
//                 rate is the group's
//   * quorum      p, then TS_QUORUM + j; proposals and votes over
//                 clocks[h], shards ascending
//   * commit      the highest proposal over all the command's shards
//                 (fantoch_ps/src/protocol/tempo.rs:614-636)
//   * events      K_h attached (keys ascending, FX_TABLE_HDR(FX_TABLE_ATTACHED,
//                 fast_quorum, key), dot, commit, the key's votes, nkeys word
//                 FX_TABLE_PS_WORD(K_h, C)) in slot i + draw(TS_WINDOW) %
//                 (window + 1); then per key index k and process q below
//                 commit on clocks[h] one detached event own + 1 .. commit in
//                 slot i + draw(TS_LAG + 16 k + q - 1) % (lag + 1)
//   * list        if C > 1: m = the command's keys at its other shards, then
//                 per other shard t ascending and key index k there
//                 FX_TABLE_TARGET(draw(TG_DELAY + 8 t + k) % (msg_lag + 1), t,
//                 key) -- the draw with the sender's a.  The attached events at
//                 h carry the list's index in route.
// A stream is its events by (slot, creation order).  The lists of a group lie
// in targets by (shard, slot of the shard's attached events, command), which
// is the order fantoch_amd.table.pack_table_groups meets them in.
//
// tg_walk is the one statement of the model.  The counting pass adds every
// event to its (shard, slot) row counter, every list's words to the (shard,
// slot) list counter and, per shard, the rows the messages to it can take;
// tg_prefix turns the counters into cursors; the emitting pass walks the same
// draws and stores.  The same function runs per lane in table_group_synth.hip
// and per group in table_synth_host.cpp.
#pragma once
#include <stdint.h>

#include "fx_table_synth.h"

namespace fx {

enum : uint64_t {
  TG_SHARDS = 37,  // a = i: shard count
  TG_COORD = 38,   // a = i: coordinator
  TG_SHARD = 64,   // a = i: + j: shard j = 0 .. 7
  TG_DELAY = 64    // a = i | (h + 1) << 32: + 8 * target shard + key index
};

// words the lists of one group cannot exceed: per command and shard of it, m
// and the keys at the other shards
inline uint64_t tg_max_list_words(const fx_table_group_synth_params& p) {
  const uint64_t scap = p.smax < p.shards ? p.smax : p.shards, kcap = p.kmax < p.keys ? p.kmax : p.keys;
  return scap > 1 ? (uint64_t)p.cmds * scap * (1u + kcap * (scap - 1u)) : 0u;
}

// rows no stream exceeds, per key of a command at a shard.  Own events: the
// attached event and one detached event per process below the commit clock.
// At one shard per command the member with the highest proposal is at the
// commit clock (n events, as ts_walk); with more shards the commit clock may
// come from another shard and all n processes are below it (n + 1).  Handled
// rows: one StableAtShard per other shard of the command on top.
inline uint64_t tg_max_rows(const fx_table_group_synth_params& p) {
  const uint64_t scap = p.smax < p.shards ? p.smax : p.shards, kcap = p.kmax < p.keys ? p.kmax : p.keys;
  return (uint64_t)p.cmds * kcap * (p.n + (scap > 1 ? 1u : 0u));
}
inline uint64_t tg_max_rows_out(const fx_table_group_synth_params& p) {
  const uint64_t scap = p.smax < p.shards ? p.smax : p.shards, kcap = p.kmax < p.keys ? p.kmax : p.keys;
  return (uint64_t)p.cmds * kcap * (scap > 1 ? p.n + scap : p.n);
}

inline int tg_check(const fx_table_group_synth_params* p) {
  if (!p || p->n < 1 || p->n > 16 || p->fast_quorum < 1 || p->fast_quorum > p->n || p->kmax < 1 ||
      p->kmax > FX_TABLE_MAX_CMD_KEYS || p->keys < 1 || p->keys > FX_TABLE_SYNTH_MAX_KEYS || p->cmds > FX_SEQ_MASK ||
      p->window > FX_SEQ_MASK || p->lag > FX_SEQ_MASK || p->num_conflicts > 8 || p->shards < 1 ||
      p->shards > FX_TABLE_MAX_CMD_SHARDS || p->smax < 1 || p->smax > FX_TABLE_MAX_CMD_SHARDS ||
      p->msg_lag > FX_TABLE_GROUP_MAX_DELAY)
    return FX_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < (p->num_conflicts ? p->num_conflicts : 1u); ++i)
    if (p->conflict_pct[i] > 100) return FX_ERR_INVALID_ARG;
  if (((uint64_t)p->group_base + p->groups) * p->shards > (1ull << 32)) return FX_ERR_INVALID_ARG;
  if ((uint64_t)p->groups * p->shards >= (1ull << 32)) return FX_ERR_INVALID_ARG;  // (num_streams is 32 bits)
  if (tg_max_rows_out(*p) >= (1ull << 26)) return FX_ERR_INVALID_ARG;  // (fx_table_run_groups' limit on rows)
  if (tg_max_list_words(*p) >= (1ull << 32)) return FX_ERR_INVALID_ARG;  // (a group's cursors are 32-bit words)
  return FX_OK;
}

// words of per-group state: clocks [shard][key][process], then the command
// counts of the coordinators
FX_HD uint32_t tg_state_words(const fx_table_group_synth_params& p) { return p.shards * p.keys * p.n + p.n; }
// delivery slots of a stream
FX_HD uint32_t tg_slots(const fx_table_group_synth_params& p) {
  return p.cmds + (p.window > p.lag ? p.window : p.lag) + 1u;
}

struct TgGroup {
  uint64_t seed, G;  // G: the global group
  uint32_t P, scap, n, fq, keys, cmds, kcap, window, lag, msg_lag, conflict, nslots;
};

FX_HD TgGroup tg_group(const fx_table_group_synth_params& p, uint32_t local) {
  TgGroup tg;
  tg.seed = p.seed;
  tg.G = (uint64_t)p.group_base + local;
  tg.P = p.shards;
  tg.scap = p.smax < p.shards ? p.smax : p.shards;
  tg.n = p.n;
  tg.fq = p.fast_quorum;
  tg.keys = p.keys;
  tg.cmds = p.cmds;
  tg.kcap = p.kmax < p.keys ? p.kmax : p.keys;
  tg.window = p.window;
  tg.lag = p.lag;
  tg.msg_lag = p.msg_lag;
  tg.nslots = tg_slots(p);
  const uint32_t nc = p.num_conflicts ? p.num_conflicts : 1;
  const uint64_t ci = p.conflict_block ? (tg.G / p.conflict_block) % nc : tg.G % nc;
  tg.conflict = p.conflict_pct[ci];
  return tg;
}

// where the emitting pass stores a group
struct TgOut {
  uint32_t *hdr, *dot, *clock, *votes, *nkeys, *route, *targets;
  size_t plane;
  uint32_t steps, twords;
  uint32_t stream0;  // the group's shard 0
};

// the keys of command i at the shard of `a`, ascending, as ts_walk picks them
FX_HD void tg_keys(const TgGroup& tg, uint64_t a, uint32_t K, uint32_t* ck) {
  constexpr uint32_t KMAX = FX_TABLE_MAX_CMD_KEYS;
  const uint32_t keys = tg.keys;
  ck[0] = (keys == 1 || (uint32_t)(synth_rand(tg.seed, tg.G, a, TS_CONFLICT) % 100u) < tg.conflict)
              ? 0u
              : 1u + (uint32_t)(synth_rand(tg.seed, tg.G, a, TS_FIRST) % (keys - 1u));
#pragma unroll
  for (uint32_t j = 1; j < KMAX; ++j) {
    ck[j] = 0xFFFFFFFFu;
    if (j < K) {
      uint32_t x = (uint32_t)(synth_rand(tg.seed, tg.G, a, TS_KEY + j) % (keys - j));
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

// state: tg_state_words words, zeroed here.  rows, lists: P * nslots words
// each, [shard][slot]; EMIT false: zero on entry, counts on return; EMIT true:
// every (shard, slot)'s first row / first targets word on entry.  extra: P
// words, EMIT false only: zero on entry; on return the rows the messages to
// each shard can take.  A row at or past o.steps and a targets word at or
// past o.twords are never stored.
template <bool EMIT>
FX_HD void tg_walk(const TgGroup& tg, const TsWords state, const TsWords rows, const TsWords lists, const TsWords extra,
                   const TgOut& o) {
  constexpr uint32_t KMAX = FX_TABLE_MAX_CMD_KEYS, PMAX = FX_TABLE_MAX_CMD_SHARDS;
  const uint32_t n = tg.n, keys = tg.keys, P = tg.P, nslots = tg.nslots;
  const uint32_t seqs = P * keys * n;
  for (uint32_t w = 0; w < seqs + n; ++w) state[w] = 0;
  for (uint32_t i = 0; i < tg.cmds; ++i) {
    // the shard set
    const uint32_t C = 1u + (uint32_t)(synth_rand(tg.seed, tg.G, i, TG_SHARDS) % tg.scap);
    uint32_t on = 0;
    for (uint32_t j = 0; j < C; ++j) {
      uint32_t r = (uint32_t)(synth_rand(tg.seed, tg.G, i, TG_SHARD + j) % (P - j));
      uint32_t h = 0;
      for (; h < P; ++h) {
        if (on >> h & 1u) continue;
        if (r == 0) break;
        --r;
      }
      on |= 1u << h;
    }
    const uint32_t p = (uint32_t)(synth_rand(tg.seed, tg.G, i, TG_COORD) % n);  // processes 0 .. n-1 in here
    const uint32_t seq = state[seqs + p] + 1u;
    state[seqs + p] = seq;
    // key counts, 4 bits per shard
    uint32_t kof = 0, ktot = 0;
    for (uint32_t h = 0; h < P; ++h)
      if (on >> h & 1u) {
        const uint64_t a = (uint64_t)i | (uint64_t)(h + 1u) << 32;
        const uint32_t K = 1u + (uint32_t)(synth_rand(tg.seed, tg.G, a, TS_COUNT) % tg.kcap);
        kof |= K << (4u * h);
        ktot += K;
      }
    // proposals shard by shard: the votes go straight to the rows
    uint32_t row0[PMAX], list0[PMAX];
    uint32_t commit = 0;
    for (uint32_t h = 0; h < P; ++h) {
      row0[h] = list0[h] = 0;
      if (!(on >> h & 1u)) continue;
      const uint64_t a = (uint64_t)i | (uint64_t)(h + 1u) << 32;
      const uint32_t K = kof >> (4u * h) & 15u;
      uint32_t ck[KMAX];
      tg_keys(tg, a, K, ck);
      uint64_t members = p;  // the quorum, 4 bits per member in pick order
      uint32_t chosen = 1u << p;
      for (uint32_t j = 1; j < tg.fq; ++j) {
        uint32_t r = (uint32_t)(synth_rand(tg.seed, tg.G, a, TS_QUORUM + j) % (n - j));
        uint32_t q = 0;
        for (; q < n; ++q) {
          if (chosen >> q & 1u) continue;
          if (r == 0) break;
          --r;
        }
        chosen |= 1u << q;
        members |= (uint64_t)q << (4u * j);
      }
      const uint32_t slot = h * nslots + i + (uint32_t)(synth_rand(tg.seed, tg.G, a, TS_WINDOW) % (tg.window + 1u));
      const uint32_t r0 = rows[slot];
      rows[slot] = r0 + K;
      row0[h] = r0;
      if (C > 1u) {
        const uint32_t l0 = lists[slot];
        lists[slot] = l0 + 1u + ktot - K;
        list0[h] = l0;
        if (!EMIT) extra[h] = extra[h] + K * (C - 1u);
      }
      const size_t base = (size_t)h * keys;
      uint32_t first = 0;
      for (uint32_t m = 0; m < tg.fq; ++m) {
        const uint32_t q = (uint32_t)(members >> (4u * m)) & 15u;
        uint32_t top = 0;
#pragma unroll
        for (uint32_t k = 0; k < KMAX; ++k)
          if (k < K) {
            const uint32_t c = state[(base + ck[k]) * n + q];
            top = c > top ? c : top;
          }
        const uint32_t prop = m == 0 || top + 1u > first ? top + 1u : first;
        if (m == 0) first = prop;
        commit = prop > commit ? prop : commit;
#pragma unroll
        for (uint32_t k = 0; k < KMAX; ++k)
          if (k < K) {
            const size_t w = (base + ck[k]) * n + q;
            if (EMIT && r0 + k < o.steps) {
              uint32_t* v = o.votes + (size_t)(3u * m) * o.plane + fx_index(r0 + k, o.stream0 + h, o.steps);
              v[0] = q + 1u;
              v[o.plane] = state[w] + 1u;
              v[2 * o.plane] = prop;
            }
            state[w] = prop;
          }
      }
    }
    // the commit clock is known: the rest of the attached events, the
    // detached votes, and this shard's keys in the other shards' lists
    uint32_t kbefore = 0;  // keys of the command at its shards below h
    for (uint32_t h = 0; h < P; ++h) {
      if (!(on >> h & 1u)) continue;
      const uint64_t a = (uint64_t)i | (uint64_t)(h + 1u) << 32;
      const uint32_t K = kof >> (4u * h) & 15u;
      uint32_t ck[KMAX];
      tg_keys(tg, a, K, ck);
      const size_t base = (size_t)h * keys;
      if (EMIT) {
#pragma unroll
        for (uint32_t k = 0; k < KMAX; ++k)
          if (k < K && row0[h] + k < o.steps) {
            const size_t at = fx_index(row0[h] + k, o.stream0 + h, o.steps);
            o.hdr[at] = FX_TABLE_HDR(FX_TABLE_ATTACHED, tg.fq, ck[k]);
            o.dot[at] = FX_PACK_DOT(p + 1u, seq);
            o.clock[at] = commit;
            o.nkeys[at] = FX_TABLE_PS_WORD(K, C);
            if (C > 1u) o.route[at] = list0[h];
          }
        if (C > 1u) {
          if (list0[h] < o.twords) o.targets[list0[h]] = ktot - K;
          for (uint32_t s = 0; s < P; ++s) {  // the senders
            if (s == h || !(on >> s & 1u)) continue;
            const uint64_t as = (uint64_t)i | (uint64_t)(s + 1u) << 32;
            const uint32_t at0 = list0[s] + 1u + kbefore - (s < h ? kof >> (4u * s) & 15u : 0u);
#pragma unroll
            for (uint32_t k = 0; k < KMAX; ++k)
              if (k < K && at0 + k < o.twords) {
                const uint32_t d = (uint32_t)(synth_rand(tg.seed, tg.G, as, TG_DELAY + 8u * h + k) % (tg.msg_lag + 1u));
                o.targets[at0 + k] = FX_TABLE_TARGET(d, h, ck[k]);
              }
          }
        }
      }
      kbefore += K;
#pragma unroll
      for (uint32_t k = 0; k < KMAX; ++k)
        if (k < K)
          for (uint32_t q = 0; q < n; ++q) {
            const size_t w = (base + ck[k]) * n + q;
            const uint32_t own = state[w];
            if (own >= commit) continue;
            state[w] = commit;
            const uint32_t ds =
                h * nslots + i + (uint32_t)(synth_rand(tg.seed, tg.G, a, TS_LAG + 16u * k + q) % (tg.lag + 1u));
            const uint32_t row = rows[ds];
            rows[ds] = row + 1u;
            if (EMIT && row < o.steps) {
              const size_t at = fx_index(row, o.stream0 + h, o.steps);
              o.hdr[at] = FX_TABLE_HDR(FX_TABLE_DETACHED, 1u, ck[k]);
              o.votes[at] = q + 1u;
              o.votes[o.plane + at] = own + 1u;
              o.votes[2 * o.plane + at] = commit;
            }
          }
    }
  }
}

// counts -> cursors.  tg_prefix_rows: an exclusive prefix over the slots of
// shard h; returns the shard's own events.  tg_list_words: the words of the
// group's lists (count = P * nslots).  tg_prefix_lists: one exclusive prefix
// over (shard, slot) from `list_base`, the group's first word in targets.
FX_HD uint32_t tg_prefix_rows(const TsWords rows, uint32_t h, uint32_t nslots) {
  uint32_t run = 0;
  for (uint32_t t = 0; t < nslots; ++t) {
    const uint32_t c = rows[h * nslots + t];
    rows[h * nslots + t] = run;
    run += c;
  }
  return run;
}
FX_HD uint32_t tg_list_words(const TsWords lists, uint32_t count) {
  uint32_t run = 0;
  for (uint32_t t = 0; t < count; ++t) run += lists[t];
  return run;
}
FX_HD void tg_prefix_lists(const TsWords lists, uint32_t count, uint32_t list_base) {
  uint32_t run = list_base;
  for (uint32_t t = 0; t < count; ++t) {
    const uint32_t c = lists[t];
    lists[t] = run;
    run += c;
  }
}

}  // namespace fx
