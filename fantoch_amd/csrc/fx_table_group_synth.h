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
// Per shard h of the set, a = i | (h + 1) << 32: the steps of a command of
// fx_table_synth.h (keys, quorum of p -- TS_COORD is not drawn --, proposals,
// attached and detached events) over clocks[h], the slots and the stream of
// shard h, the conflict rate the group's, but for
//   * commit      the highest proposal over all the command's shards
//                 (fantoch_ps/src/protocol/tempo.rs:614-636), shards ascending
//   * nkeys word  FX_TABLE_PS_WORD(K_h, C)
//   * list        if C > 1: m = the command's keys at its other shards, then
//                 per other shard t ascending and key index k there
//                 FX_TABLE_TARGET(draw(TG_DELAY + 8 t + k) % (msg_lag + 1), t,
//                 key) -- the draw with the sender's a.  The attached events at
//                 h carry the list's index in route.
// A stream is its events by (slot, creation order).  The lists of a group lie
// in targets by (shard, slot of the shard's attached events, command), which
// is the order fantoch_amd.table.pack_table_groups meets them in.
//
// tg_walk: the counting pass adds every event to its (shard, slot) row
// counter, every list's words to the (shard, slot) list counter and, per
// shard, the rows the messages to it can take; ts_prefix per shard and
// tg_prefix_lists turn the counters into cursors; the emitting pass walks the
// same draws and stores.  The same function runs per lane in
// table_group_synth.hip and per group in table_synth_host.cpp.
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
  if (!p || !ts_common_ok(*p) || p->shards < 1 || p->shards > FX_TABLE_MAX_CMD_SHARDS || p->smax < 1 ||
      p->smax > FX_TABLE_MAX_CMD_SHARDS || p->msg_lag > FX_TABLE_GROUP_MAX_DELAY)
    return FX_ERR_INVALID_ARG;
  if (((uint64_t)p->group_base + p->groups) * p->shards > (1ull << 32)) return FX_ERR_INVALID_ARG;
  if ((uint64_t)p->groups * p->shards >= (1ull << 32)) return FX_ERR_INVALID_ARG;  // (num_streams is 32 bits)
  if (tg_max_rows_out(*p) >= (1ull << 26)) return FX_ERR_INVALID_ARG;  // (fx_table_run_groups' limit on rows)
  if (tg_max_list_words(*p) >= (1ull << 32)) return FX_ERR_INVALID_ARG;  // (a group's cursors are 32-bit words)
  return FX_OK;
}

// words of per-group state: clocks [shard][key][process], then the command
// counts of the coordinators
FX_HD uint32_t tg_state_words(const fx_table_group_synth_params& p) { return p.shards * p.keys * p.n + p.n; }

struct TgGroup {
  TsStream ts;  // ts.g: the global group
  uint32_t P, scap, msg_lag, nslots;
};

FX_HD TgGroup tg_group(const fx_table_group_synth_params& p, uint32_t local) {
  TgGroup tg;
  tg.ts = ts_model(p, (uint64_t)p.group_base + local);
  tg.P = p.shards;
  tg.scap = p.smax < p.shards ? p.smax : p.shards;
  tg.msg_lag = p.msg_lag;
  tg.nslots = ts_slots(p);
  return tg;
}

// where the emitting pass stores a group (ev.stream: the group's shard 0)
struct TgOut {
  TsOut ev;
  uint32_t *route, *targets;
  uint32_t twords;
};

// the draws of command i at shard h
FX_HD TsDraw tg_draw(const TsStream& ts, uint32_t i, uint32_t h) {
  return TsDraw{ts.seed, ts.g, (uint64_t)i | (uint64_t)(h + 1u) << 32};
}

// state: tg_state_words words, zeroed here.  rows, lists: P * nslots words
// each, [shard][slot]; EMIT false: zero on entry, counts on return; EMIT true:
// every (shard, slot)'s first row / first targets word on entry.  extra: P
// words, EMIT false only: zero on entry; on return the rows the messages to
// each shard can take.  A row at or past o.ev.steps and a targets word at or
// past o.twords are never stored.
template <bool EMIT>
FX_HD void tg_walk(const TgGroup& tg, const TsWords state, const TsWords rows, const TsWords lists, const TsWords extra,
                   const TgOut& o) {
  constexpr uint32_t KMAX = FX_TABLE_MAX_CMD_KEYS, PMAX = FX_TABLE_MAX_CMD_SHARDS;
  const TsStream& ts = tg.ts;
  const uint32_t n = ts.n, keys = ts.keys, P = tg.P, nslots = tg.nslots;
  const uint32_t seqs = P * keys * n;
  for (uint32_t w = 0; w < seqs + n; ++w) state[w] = 0;
  for (uint32_t i = 0; i < ts.cmds; ++i) {
    const TsDraw cmd{ts.seed, ts.g, i};
    // the shard set
    const uint32_t C = 1u + cmd(TG_SHARDS, tg.scap);
    uint32_t on = 0;
    for (uint32_t j = 0; j < C; ++j) on |= 1u << ts_pick_free(on, cmd(TG_SHARD + j, P - j), P);
    const uint32_t p = cmd(TG_COORD, n);  // processes 0 .. n-1 in here
    const uint32_t seq = state[seqs + p] + 1u;
    state[seqs + p] = seq;
    // key counts, 4 bits per shard
    uint32_t kof = 0, ktot = 0;
    for (uint32_t h = 0; h < P; ++h)
      if (on >> h & 1u) {
        const uint32_t K = 1u + tg_draw(ts, i, h)(TS_COUNT, ts.kcap);
        kof |= K << (4u * h);
        ktot += K;
      }
    // proposals shard by shard: the votes go straight to the rows
    uint32_t row0[PMAX], list0[PMAX];
    uint32_t commit = 0;
    for (uint32_t h = 0; h < P; ++h) {
      row0[h] = list0[h] = 0;
      if (!(on >> h & 1u)) continue;
      const TsDraw draw = tg_draw(ts, i, h);
      const uint32_t K = kof >> (4u * h) & 15u;
      uint32_t ck[KMAX];
      ts_pick_keys(draw, keys, ts.conflict, K, ck);
      const uint64_t members = ts_pick_quorum(draw, p, n, ts.fq);
      const uint32_t slot = h * nslots + i + draw(TS_WINDOW, ts.window + 1u);
      const uint32_t r0 = rows[slot];
      rows[slot] = r0 + K;
      row0[h] = r0;
      if (C > 1u) {
        const uint32_t l0 = lists[slot];
        lists[slot] = l0 + 1u + ktot - K;
        list0[h] = l0;
        if (!EMIT) extra[h] = extra[h] + K * (C - 1u);
      }
      const uint32_t top =
          ts_propose<EMIT>(state.from((size_t)h * keys * n), n, ts.fq, members, K, ck, r0, o.ev, o.ev.stream + h);
      commit = top > commit ? top : commit;
    }
    // the commit clock is known: the rest of the attached events, the
    // detached votes, and this shard's keys in the other shards' lists
    uint32_t kbefore = 0;  // keys of the command at its shards below h
    for (uint32_t h = 0; h < P; ++h) {
      if (!(on >> h & 1u)) continue;
      const TsDraw draw = tg_draw(ts, i, h);
      const uint32_t K = kof >> (4u * h) & 15u;
      uint32_t ck[KMAX];
      ts_pick_keys(draw, keys, ts.conflict, K, ck);
      ts_emit_attached<EMIT>(o.ev, o.ev.stream + h, row0[h], K, ck, ts.fq, FX_PACK_DOT(p + 1u, seq), commit,
                             FX_TABLE_PS_WORD(K, C), C > 1u ? o.route : nullptr, list0[h]);
      if (EMIT && C > 1u) {
        if (list0[h] < o.twords) o.targets[list0[h]] = ktot - K;
        for (uint32_t s = 0; s < P; ++s) {  // the senders
          if (s == h || !(on >> s & 1u)) continue;
          const TsDraw sender = tg_draw(ts, i, s);
          const uint32_t at0 = list0[s] + 1u + kbefore - (s < h ? kof >> (4u * s) & 15u : 0u);
#pragma unroll
          for (uint32_t k = 0; k < KMAX; ++k)
            if (k < K && at0 + k < o.twords)
              o.targets[at0 + k] = FX_TABLE_TARGET(sender(TG_DELAY + 8u * h + k, tg.msg_lag + 1u), h, ck[k]);
        }
      }
      kbefore += K;
#pragma unroll
      for (uint32_t k = 0; k < KMAX; ++k)
        if (k < K)
          ts_detach<EMIT>(draw, state.from((size_t)h * keys * n), rows.from((size_t)h * nslots), n, i, ts.lag, k, ck[k],
                          commit, o.ev, o.ev.stream + h);
    }
  }
}

// counts -> cursors: the rows of shard h by ts_prefix over
// rows.from(h * nslots), which returns the shard's own events.  tg_list_words:
// the words of the group's lists (count = P * nslots).  tg_prefix_lists: one
// exclusive prefix over (shard, slot) from `list_base`, the group's first word
// in targets.
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
