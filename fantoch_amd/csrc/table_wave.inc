// table_wave.inc -- the body of a table executor kernel (table_exec.hip): one
// wavefront runs one stream.  Included into k_table, whose template parameters
// HBM, R, WPB, MULTI, SHARDS and RESUME it reads with GROUP = false, and into
// k_table_group (GROUP = true: the HBM _ps executor), with the kernel's
// arguments `a` (TArgs) and `ga` (GArgs, read in a group only).  A second
// kernel cannot share the body through a function: the kernels of k_table
// then compile to other code than they did, kernel arguments being what they
// are to the compiler only in the kernel itself.
  static_assert(!RESUME || (HBM && R == TS_R && WPB == 1), "resumable streams keep their tables in `state`");
  static_assert(!GROUP || (HBM && WPB == 1 && MULTI && SHARDS && !RESUME), "a group runs the HBM _ps executor");
  constexpr uint32_t KIND = SHARDS ? FX_TABLE_KIND_PS : MULTI ? FX_TABLE_KIND_MK : FX_TABLE_KIND_SINGLE;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const uint32_t wv = (WPB > 1 || GROUP) ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0u;
  // GROUP: workgroup w is group w, wavefront h its shard h, stream w * shards + h
  const uint32_t li = xcd_slot(blockIdx.x) * (GROUP ? ga.shards : WPB) + wv;
  if (GROUP ? xcd_slot(blockIdx.x) >= ga.groups : li >= a.num_lanes) return;  // whole wavefront (GROUP: workgroup)
  const uint32_t lid = threadIdx.x & 63u;
  const uint32_t s = (!GROUP && a.stream_map) ? a.stream_map[li] : li;
  const uint32_t osteps = GROUP ? ga.steps_out : a.steps;  // rows of the output planes
  const uint32_t n = a.n, keys = a.keys;
  const bool vlane = lid < NV;
  const bool at_commit = (a.flags & FX_FLAG_EXECUTE_AT_COMMIT) != 0;
  constexpr bool BMEM = HBM && SHARDS;  // stable_shards_buffered in `state`
  constexpr uint32_t BN = FX_TABLE_PS_HBM_BUFFERED, BROWS = BN / 64u;
  uint32_t* const g = !HBM ? nullptr
                      : RESUME ? a.state + (size_t)li * ts_stride(KIND, keys)
                               : a.state + (size_t)li * (hbm_words(keys) + (BMEM ? 3u * BN : 0u));
  // [e] key, [BN + e] dot, [2 * BN + e] count (0 = free) of entry e = row * 64 + lane
  uint32_t* const gb = BMEM ? g + hbm_words(keys) : nullptr;
  (void)gb;
  uint32_t* const img = RESUME ? g + ts_image_at(KIND, keys) : nullptr;
  (void)img;
  const bool init = !RESUME || (a.flags & FX_FLAG_INIT) != 0;
  uint32_t hv = 0;  // RESUME: the header words, word w on lane w
  (void)hv;
  if constexpr (RESUME) {
    if (!init) {
      const uint32_t len = a.lengths ? min(a.lengths[s], a.steps) : a.steps;
      hv = img[ts_hdr(lid)];
      // the session contract; then a stream that stopped stays stopped, and one
      // with no new rows is done: nothing but err and nexec is written
      const bool same = rl(hv, TS_H_STEPS) == a.steps && rl(hv, TS_H_N) == n && rl(hv, TS_H_KEYS) == keys &&
                        rl(hv, TS_H_VMAX) == a.vmax && rl(hv, TS_H_THR) == a.thr && rl(hv, TS_H_KIND) == KIND &&
                        rl(hv, TS_H_AT_COMMIT) == (at_commit ? 1u : 0u);
      const uint32_t was = same ? rl(hv, TS_H_ERR) : (uint32_t)FX_ERR_INVALID_ARG;
      const uint32_t dn = rl(hv, TS_H_DONE);
      if (was || len <= dn) {
        if (lid == 0) {
          a.nexec[s] = rl(hv, TS_H_NEXEC);
          a.err[s] = was ? was : len < dn ? (uint32_t)FX_ERR_INVALID_ARG : 0u;
        }
        return;
      }
    }
  }
  if constexpr (BMEM)
    if (init)
      for (uint32_t j = 0; j < BROWS; ++j) gb[2u * BN + j * 64u + lid] = 0;
  // ONCHIP: key k's row = 32 words, [lb + k * 32 + v] frontier, [+ 16 + v] window
  const uint32_t lb = wv * keys * 32u;
  if (vlane && init) {
    if constexpr (HBM) {
      for (size_t j = 0; j < (size_t)keys * (1u + WB); ++j) g[j * NV + lid] = 0;
    } else {
      for (uint32_t k = 0; k < keys; ++k) {
        smem[lb + k * 32u + lid] = 0;
        smem[lb + k * 32u + 16u + lid] = 0;
      }
    }
  }
  uint32_t pk[R], pc[R], pd[R], pa[R];
#pragma unroll
  for (uint32_t i = 0; i < R; ++i) pk[i] = NONE, pc[i] = 0, pd[i] = 0, pa[i] = 0;
  uint32_t nexec = 0, err = 0;
  const uint32_t len = a.lengths ? min(a.lengths[s], a.steps) : a.steps;

  // ---- MULTI: queues, stable counts, to_executors, stable_shards_buffered
  constexpr uint32_t SC = 64u * R;  // ring entries: entry e at lane e & 63, row (e >> 6) % R
  uint32_t pm[R], sk[R], sd[R];     // op meta; ring of (key, dot)
#pragma unroll
  for (uint32_t i = 0; i < R; ++i) pm[i] = 0, sk[i] = 0, sd[i] = 0;
  uint32_t bk = 0, bd = 0, bc = 0;  // one buffered (key, dot, count) per lane, free while bc == 0
  uint32_t bhi = 0;                 // BMEM: rows of the table in `state` that were ever used
  (void)bhi;
  uint32_t pz[R];  // SHARDS: missing_stable_shards | shards << 8
#pragma unroll
  for (uint32_t i = 0; i < R; ++i) pz[i] = 0;
  uint32_t qseq = 0, mb = 0, mt = 0, nbuf = 0, step = 0;  // messages [mb, mt) are on to_executors
  uint32_t start = 0;  // the first row of this call
  // GROUP: this shard's inbox and send list, every shard's counts (the layout at GI above)
  const uint32_t P = GROUP ? ga.shards : 1u;
  uint32_t* const ginbox = GROUP ? smem + wv * 4u * GI : nullptr;
  uint32_t* const gsends = GROUP ? smem + P * 4u * GI : nullptr;  // shard f's list at [f * 4 * GS]
  uint32_t* const gsend = GROUP ? gsends + wv * 4u * GS : nullptr;
  uint32_t* const gcount = GROUP ? gsends + P * 4u * GS : nullptr;  // [f] sends, [P + f] events left
  uint32_t nsend = 0;  // sends of this round
  (void)ginbox, (void)gsend, (void)gcount, (void)nsend;
  if constexpr (RESUME) {
    if (!init) {
      start = rl(hv, TS_H_DONE);
      nexec = rl(hv, TS_H_NEXEC);
#pragma unroll
      for (uint32_t i = 0; i < R; ++i) {
        pk[i] = img[ts_reg(TS_P_KEY, i, lid)], pc[i] = img[ts_reg(TS_P_CLOCK, i, lid)];
        pd[i] = img[ts_reg(TS_P_DOT, i, lid)], pa[i] = img[ts_reg(TS_P_ARRIVAL, i, lid)];
        if constexpr (MULTI) {
          pm[i] = img[ts_reg(TS_P_META, i, lid)];
          sk[i] = img[ts_reg(TS_P_RING_KEY, i, lid)], sd[i] = img[ts_reg(TS_P_RING_DOT, i, lid)];
        }
        if constexpr (SHARDS) pz[i] = img[ts_reg(TS_P_SHARDS, i, lid)];
      }
      if constexpr (MULTI) {
        qseq = rl(hv, TS_H_QSEQ), mb = rl(hv, TS_H_MB), mt = rl(hv, TS_H_MT), nbuf = rl(hv, TS_H_NBUF);
        if constexpr (SHARDS) bhi = rl(hv, TS_H_BHI);
        else bk = img[ts_buf(0, lid)], bd = img[ts_buf(1, lid)], bc = img[ts_buf(2, lid)];
      }
    }
  }

  // do_execute (executor.rs:365-380) of the one op selected by hit[]; SHARDS:
  // ha is its event row, wave-uniform, so one lane stores and the addresses
  // are scalar work (R address pairs per call site cost the HBM kernel its
  // second wave per SIMD)
  auto execute_hit = [&](const bool (&hit)[R], uint32_t ha) __attribute__((always_inline)) {
    if constexpr (SHARDS) {
      if (lid == 0) {
        a.order[fx_index(nexec, s, osteps)] = ha | FX_ORDER_SCC_START;
        a.release[fx_index(ha, s, osteps)] = step;
      }
#pragma unroll
      for (uint32_t i = 0; i < R; ++i)
        if (hit[i]) pk[i] = NONE;
    } else {
      (void)ha;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i) {
        if (hit[i]) {
          a.order[fx_index(nexec, s, osteps)] = pa[i] | FX_ORDER_SCC_START;
          a.release[fx_index(pa[i], s, osteps)] = step;
          pk[i] = NONE;
        }
      }
    }
    ++nexec;
  };
  // tries the ops of key k's queue from its head until one is handed back
  // (the loops of executor.rs:198-217 and :250-276 around :280-359)
  auto run_queue = [&](uint32_t k) __attribute__((always_inline)) {
    for (;;) {
      uint32_t lo = NONE;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i)
        if (pk[i] == k && m_state(pm[i]) != ST_TABLE) lo = min(lo, pm[i] & SEQ_MASK);
      lo = wave_min(lo);
      if (lo == NONE) return;  // the queue is empty
      bool hit[R];
      uint32_t hm = 0, hd = 0, hz = 0, ha = 0;  // SHARDS: the head's second word and event row
      (void)hz;
      (void)ha;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i) {
        hit[i] = pk[i] == k && m_state(pm[i]) != ST_TABLE && (pm[i] & SEQ_MASK) == lo;
        const uint64_t b = __ballot(hit[i]);
        if (b) hm = rl(pm[i], (uint32_t)__builtin_ctzll(b)), hd = rl(pd[i], (uint32_t)__builtin_ctzll(b));
        if constexpr (SHARDS)
          if (b) hz = rl(pz[i], (uint32_t)__builtin_ctzll(b)), ha = rl(pa[i], (uint32_t)__builtin_ctzll(b));
      }
      if (m_state(hm) != ST_QUEUED) return;  // the head tried before and waits for its StableAtShard
      const uint32_t K = m_nkeys(hm);
      if (K == 1 && (!SHARDS || (hz >> 8) == 1u)) {  // :290-293 (:71-75: one key, one shard)
        execute_hit(hit, ha);
        continue;
      }
      // :319-322: one more op of the command tried (SHARDS with one key here,
      // :311-316: the count is 1 = K at once and there is no other key to tell)
      uint32_t cnt = 0;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i) {
        if (hit[i]) pm[i] = m_with(pm[i], ST_TRIED);
        cnt += (uint32_t)__builtin_popcountll(__ballot(pk[i] != NONE && pd[i] == hd && m_state(pm[i]) == ST_TRIED));
      }
      uint32_t missing = 1;
      bool sends = false;  // this try ran send_stable_msg (:296-309)
      (void)sends;
      if constexpr (SHARDS) missing = hz & 0xFFu;
      if (cnt == K) {  // :328-341: the other keys are told, ascending (DESIGN.md C13)
        if constexpr (GROUP)
          if ((hz >> 8) > 1u && nsend >= GS) { err = FX_ERR_CAPACITY; return; }  // (as the ring below)
        for (uint32_t j = 1; j < K; ++j) {
          uint32_t ok = NONE;
#pragma unroll
          for (uint32_t i = 0; i < R; ++i)
            if (pk[i] != NONE && pk[i] != k && pd[i] == hd && m_state(pm[i]) == ST_TRIED) ok = min(ok, pk[i]);
          ok = wave_min(ok);
          if (ok == NONE) break;  // (nkeys - 1 other ops tried: there is one)
          if (mt - mb >= SC) { err = FX_ERR_CAPACITY; return; }
          const uint32_t e = mt % SC;
#pragma unroll
          for (uint32_t i = 0; i < R; ++i) {
            if (pk[i] == ok && pd[i] == hd && m_state(pm[i]) == ST_TRIED) pm[i] = m_with(pm[i], ST_TOLD);
            if ((e >> 6) == i && lid == (e & 63u)) sk[i] = ok, sd[i] = hd;
          }
          ++mt;
        }
        if constexpr (SHARDS) --missing, sends = true;  // :316, :333
        else missing = 0;
      }
      if (nbuf) {  // :345-347
        if constexpr (BMEM) {
          for (uint32_t j = 0; j < bhi; ++j) {
            const uint32_t o = j * 64u + lid, oc = gb[2u * BN + o];
            const uint64_t b = __ballot(oc != 0 && gb[o] == k && gb[BN + o] == hd);
            if (b) {
              const uint32_t l = (uint32_t)__builtin_ctzll(b), c = rl(oc, l);
              if (c > missing) { err = FX_ERR_INVALID_ARG; return; }  // (before anything of this try is written)
              missing -= c;
              if (lid == l) gb[2u * BN + o] = 0;
              --nbuf;
              break;
            }
          }
        } else {
          const uint64_t b = __ballot(bc != 0 && bk == k && bd == hd);
          if (b) {
            const uint32_t l = (uint32_t)__builtin_ctzll(b);
            if constexpr (SHARDS)
              if (rl(bc, l) > missing) { err = FX_ERR_INVALID_ARG; return; }  // (before anything of this try is written)
            missing -= rl(bc, l);
            if (lid == l) bc = 0;
            --nbuf;
          }
        }
      }
      if constexpr (SHARDS) {
#pragma unroll
        for (uint32_t i = 0; i < R; ++i) {
          if (hit[i]) {
            pz[i] = (pz[i] & ~0xFFu) | missing;
            if (sends) pm[i] = m_with(pm[i], ST_TOLD);
          }
        }
        if (sends && a.sent && lid == 0) a.sent[fx_index(ha, s, osteps)] = step;
        if constexpr (GROUP) {
          // the send list of the round: the route is that of the own event in
          // handled row ha, which lane 0 stored into handled_src and reads back
          if (sends && (hz >> 8) > 1u) {
            if (lid == 0) {
              const uint32_t own = ga.hsrc[fx_index(ha, s, osteps)];
              uint32_t* const e = gsend + nsend;
              e[0] = step, e[GS] = ha, e[2u * GS] = ga.route[fx_index(own, s, a.steps)], e[3u * GS] = hd;
            }
            ++nsend;
          }
        }
      }
      if (missing != 0) return;  // :353-357: handed back, it stays the head
      execute_hit(hit, ha);      // :349-352
    }
  };
  // handle_stable_msg (executor.rs:168-235)
  auto stable_msg = [&](uint32_t k, uint32_t d) __attribute__((always_inline)) {
    uint32_t lo = NONE;
#pragma unroll
    for (uint32_t i = 0; i < R; ++i)
      if (pk[i] == k && m_state(pm[i]) != ST_TABLE) lo = min(lo, pm[i] & SEQ_MASK);
    lo = wave_min(lo);
    bool hit[R];
    uint64_t any = 0;
#pragma unroll
    for (uint32_t i = 0; i < R; ++i) {
      hit[i] = pk[i] == k && m_state(pm[i]) != ST_TABLE && (pm[i] & SEQ_MASK) == lo && pd[i] == d;
      any |= __ballot(hit[i]);
    }
    if (lo != NONE && any) {  // :173-217: missing_stable_shards 1 -> 0
      uint32_t ha = 0;
      if constexpr (SHARDS) {     // :177-186: one off, the head executes at 0
        uint32_t z = 0;
#pragma unroll
        for (uint32_t i = 0; i < R; ++i) {
          const uint64_t b = __ballot(hit[i]);
          if (b) z = rl(pz[i], (uint32_t)__builtin_ctzll(b)), ha = rl(pa[i], (uint32_t)__builtin_ctzll(b));
        }
        if ((z & 0xFFu) != 1u) {
#pragma unroll
          for (uint32_t i = 0; i < R; ++i)
            if (hit[i]) pz[i] -= 1u;
          return;
        }
      }
      execute_hit(hit, ha);
      run_queue(k);
      return;
    }
    // :219-233
    if constexpr (BMEM) {
      for (uint32_t j = 0; j < bhi; ++j) {
        const uint32_t o = j * 64u + lid, oc = gb[2u * BN + o];
        const uint64_t b = __ballot(oc != 0 && gb[o] == k && gb[BN + o] == d);
        if (b) {
          if (lid == (uint32_t)__builtin_ctzll(b)) gb[2u * BN + o] = oc + 1u;
          return;
        }
      }
      for (uint32_t j = 0; j < BROWS; ++j) {
        const uint32_t o = j * 64u + lid;
        const uint64_t fr = __ballot(gb[2u * BN + o] == 0);
        if (fr) {
          if (lid == (uint32_t)__builtin_ctzll(fr)) gb[o] = k, gb[BN + o] = d, gb[2u * BN + o] = 1;
          bhi = max(bhi, j + 1u);
          ++nbuf;
          return;
        }
      }
      err = FX_ERR_CAPACITY;
      return;
    }
    const uint64_t b = __ballot(bc != 0 && bk == k && bd == d);
    if (b) {
      if (lid == (uint32_t)__builtin_ctzll(b)) ++bc;
      return;
    }
    const uint64_t fr = __ballot(bc == 0);
    if (!fr) { err = FX_ERR_CAPACITY; return; }
    if (lid == (uint32_t)__builtin_ctzll(fr)) bk = k, bd = d, bc = 1;
    ++nbuf;
  };
  // the runner's drain after an event (fantoch/src/sim/runner.rs:411-416): the
  // messages on to_executors now, last pushed first, each handled once; what
  // the handlers push waits for the next event's drain.  It runs before the
  // next event is looked at, and once after the last.
  auto drain = [&]() __attribute__((always_inline)) {
    const uint32_t top = mt;
    for (uint32_t e = top; e != mb && !err;) {
      --e;
      const uint32_t x = e % SC;
      uint32_t mk = 0, md = 0;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i)
        if ((x >> 6) == i) mk = rl(sk[i], x & 63u), md = rl(sd[i], x & 63u);
      stable_msg(mk, md);
    }
    mb = top;
  };

  // the inputs of the 4-step tile row holding step r0: lane 4q + k holds step
  // r0 + k of plane q -- 0 hdr, 1 dot, 2 clock, 3 + p vote plane p (p < 12:
  // the first four vote slots) -- one load, issued a row ahead of its use
  auto row_load = [&](uint32_t r0) -> uint32_t {
    const uint32_t q = lid >> 2;
    const size_t at = fx_index(r0 + (lid & 3u), s, a.steps);
    if (q == 0) return a.hdr[at];
    if (q == 1) return a.dot[at];
    if (q == 2) return a.clock[at];
    const uint32_t p = q - 3u;
    if constexpr (MULTI)
      if (q == 15u) return a.nkeys[at];  // lanes 60..63
    return (q < 15u && p < 3u * a.vmax) ? a.votes[(size_t)p * a.plane + at] : 0u;
  };
  // (a resumed call starts inside a tile row: that row first)
  const uint32_t row0 = start & ~3u;
  uint32_t row = len ? row_load(row0) : 0u, next = len > row0 + 4 ? row_load(row0 + 4) : 0u;

  // One event (table_event.inc): here the body of the loop over the stream's
  // rows; in a group a callable unit that returns to the round loop.
  if constexpr (!GROUP) {
    for (uint32_t r = start; r < len; ++r) {
      if constexpr (MULTI) {
        // of the event before (events that `continue` push nothing).  The call
        // before a resumed one ended with the drain of its last event: what that
        // pushed waits for the drain of this call's first
        if (!RESUME || r != start) drain();
        if (err) break;
        step = r;
      }
      if (r != start && !(r & 3u)) {
        row = next;
        if (r + 4 < len) next = row_load(r + 4);
      }
      const uint32_t hj = r;
#define FX_EVENT_NEXT continue
#define FX_EVENT_STOP break
#include "table_event.inc"
#undef FX_EVENT_NEXT
#undef FX_EVENT_STOP
    }
    if constexpr (MULTI)
      if (!err) drain();
  } else {
    auto event = [&](uint32_t r, uint32_t hj) __attribute__((always_inline)) {
#define FX_EVENT_NEXT return
#define FX_EVENT_STOP return
#include "table_event.inc"
#undef FX_EVENT_NEXT
#undef FX_EVENT_STOP
    };
    // The closed loop of the group (DESIGN.md C14), one round per iteration.
    // In round t this shard handles the messages of its inbox due at or before
    // t, ascending by (due round, send index), then its own event t; every
    // handled event takes the next row j of the output planes.  After the
    // round's barrier every wavefront walks the send lists of shards 0..P-1,
    // each ascending by (step, handled row), and expands the targets: every
    // message takes the next send index -- the same walk in every wavefront,
    // so the same count, without atomics -- and each wavefront keeps those for
    // its own shard.  A second barrier ends the round: the lists are free and
    // the "events left" words are set.
    // Barriers: the loop leaves only where every wavefront of the workgroup
    // reads the same LDS words or kernel arguments after a barrier (no shard
    // has events left; the cap on rounds), and the two barriers of a round are
    // in the loop's own body, outside every lambda and every branch on a
    // wavefront's own state, so all wavefronts meet both in every round.
    err = rl(a.err[s], 0);  // the input check's verdict: such a stream never starts
#pragma unroll
    for (uint32_t i = 0; i < GI / 64u; ++i) ginbox[i * 64u + lid] = NONE;
    uint32_t j = 0, inb = 0, gidx = 0, t = 0;  // handled rows, messages in the inbox, the group's send index, round
    // the next handled row: a message (src = FX_TABLE_HANDLED_MSG | key, its
    // dot) or the own event in input row r (src = r).  A stream that stopped
    // earlier in the round still lists the round's events, as the host-paced
    // loop does (fantoch_amd.table.run_table_groups feeds a round in one call)
    auto handle = [&](uint32_t src, uint32_t d, uint32_t r) __attribute__((always_inline)) {
      if (j >= osteps) {
        if (!err) err = FX_ERR_ORDER_OVERFLOW;
        return;
      }
      if (lid == 0) {
        const size_t oat = fx_index(j, s, osteps);
        ga.hsrc[oat] = src, ga.hdot[oat] = d;
        a.release[oat] = NONE, a.sent[oat] = NONE;
      }
      // (other lanes store into this release row when the event's op executes)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      const uint32_t row_j = j++;
      if (err) return;
      step = row_j;
      if (src & FX_TABLE_HANDLED_MSG) {
        if (!at_commit) stable_msg(src & TGT_KEY, d);
      } else {
        event(r, row_j);
      }
      if (!err) drain();  // what this event pushed: its sends belong to this round
    };
    if (lid == 0) gcount[P + wv] = (!err && len) ? 1u : 0u;
    __syncthreads();
    for (;;) {
      uint32_t any = 0;
      for (uint32_t f = 0; f < P; ++f) any |= gcount[P + f];
      if (!any) break;  // (the same words in every wavefront)
      if (t >= ga.max_rounds) {
        if (gcount[P + wv]) err = FX_ERR_INVALID_ARG;
        break;  // (the same t and cap in every wavefront)
      }
      nsend = 0;
      if (!err) {
        bool own = t < len;  // the own event of the round is still to come
        for (;;) {
          uint32_t src = t, d = 0, due = NONE;
          if (inb) {
#pragma unroll
            for (uint32_t i = 0; i < GI / 64u; ++i) due = min(due, ginbox[i * 64u + lid]);
            due = wave_min(due);
          }
          if (due <= t) {
            uint32_t ix = NONE;
#pragma unroll
            for (uint32_t i = 0; i < GI / 64u; ++i)
              if (ginbox[i * 64u + lid] == due) ix = min(ix, ginbox[GI + i * 64u + lid]);
            ix = wave_min(ix);
#pragma unroll
            for (uint32_t i = 0; i < GI / 64u; ++i) {
              const uint32_t e = i * 64u + lid;
              const bool me = ginbox[e] == due && ginbox[GI + e] == ix;
              const uint64_t b = __ballot(me);
              if (b) {
                const uint32_t l = (uint32_t)__builtin_ctzll(b);
                src = FX_TABLE_HANDLED_MSG | rl(ginbox[2u * GI + e], l), d = rl(ginbox[3u * GI + e], l);
                if (me) ginbox[e] = NONE;
              }
            }
            --inb;
          } else if (own) {
            own = false;
            if (t != 0 && !(t & 3u) && !err) {
              row = next;
              if (t + 4 < len) next = row_load(t + 4);
            }
          } else {
            break;
          }
          handle(src, d, t);
        }
      }
      if (lid == 0) gcount[wv] = nsend;
      __syncthreads();
      for (uint32_t f = 0; f < P; ++f) {
        const uint32_t cnt = gcount[f];
        if (!cnt || f == wv) {  // (nothing of a shard's own sends is for itself; the count goes on)
          for (uint32_t q = 0; q < cnt; ++q) gidx += ga.targets[gsends[f * 4u * GS + 2u * GS + q]];
          continue;
        }
        const uint32_t* const fs = gsends + f * 4u * GS;
        const bool on = lid < cnt;
        const uint32_t es = on ? fs[lid] : 0u, er = on ? fs[GS + lid] : 0u;
        const uint32_t ert = on ? fs[2u * GS + lid] : 0u, ed = on ? fs[3u * GS + lid] : 0u;
        uint32_t rank = 0;  // within one step the tries' order is not row order
        for (uint32_t q = 0; q < cnt; ++q) {
          const uint32_t qs = rl(es, q), qr = rl(er, q);
          rank += (qs < es || (qs == es && qr < er)) ? 1u : 0u;
        }
        for (uint32_t q = 0; q < cnt; ++q) {
          const uint32_t l = (uint32_t)__builtin_ctzll(__ballot(on && rank == q));
          const uint32_t rt = rl(ert, l), d = rl(ed, l);
          const uint32_t m = rl(ga.targets[rt], 0);
          for (uint32_t base = 0; base < m; base += 64u) {
            const bool in = base + lid < m;
            const uint32_t w = in ? ga.targets[rt + 1u + base + lid] : 0u;
            for (uint64_t b = __ballot(in && tgt_shard(w) == wv); b && !err; b &= b - 1u) {
              const uint32_t x = (uint32_t)__builtin_ctzll(b), xw = rl(w, x);
              if (inb >= GI) { err = FX_ERR_CAPACITY; break; }
              bool placed = false;
#pragma unroll
              for (uint32_t i = 0; i < GI / 64u; ++i) {
                if (!placed) {
                  const uint32_t e = i * 64u + lid;
                  const uint64_t fr = __ballot(ginbox[e] == NONE);
                  if (fr) {
                    if (lid == (uint32_t)__builtin_ctzll(fr)) {
                      ginbox[e] = t + 1u + tgt_delay(xw), ginbox[GI + e] = gidx + base + x;
                      ginbox[2u * GI + e] = xw & TGT_KEY, ginbox[3u * GI + e] = d;
                    }
                    placed = true;
                  }
                }
              }
              ++inb;
            }
          }
          gidx += m;
        }
      }
      if (err) inb = 0;  // a stopped shard handles nothing more; messages to it are dropped
      ++t;
      if (lid == 0) gcount[P + wv] = (!err && (t < len || inb)) ? 1u : 0u;
      __syncthreads();
    }
    if (lid == 0) {
      ga.hlen[s] = j;
      if (wv == 0) ga.rounds[xcd_slot(blockIdx.x)] = t;
    }
  }

  if (a.stable) {
    for (uint32_t k = 0; k < keys; ++k) {
      uint32_t f = 0;
      if (vlane) {
        if constexpr (HBM) f = g[(size_t)k * NV + lid];
        else f = smem[lb + k * 32u + lid];
      }
      const uint32_t sc = stable_of(f, n, a.thr, lid);
      if (lid == 0) a.stable[(size_t)s * keys + k] = sc;
    }
  }
  if (lid == 0) {
    a.nexec[s] = nexec;
    a.err[s] = err;
  }
  if constexpr (RESUME) {
    if (lid == 0) {
      img[ts_hdr(TS_H_STEPS)] = a.steps, img[ts_hdr(TS_H_N)] = n, img[ts_hdr(TS_H_KEYS)] = keys;
      img[ts_hdr(TS_H_VMAX)] = a.vmax, img[ts_hdr(TS_H_THR)] = a.thr, img[ts_hdr(TS_H_KIND)] = KIND;
      img[ts_hdr(TS_H_AT_COMMIT)] = at_commit ? 1u : 0u;
      img[ts_hdr(TS_H_DONE)] = len, img[ts_hdr(TS_H_NEXEC)] = nexec, img[ts_hdr(TS_H_ERR)] = err;
      img[ts_hdr(TS_H_QSEQ)] = qseq, img[ts_hdr(TS_H_MB)] = mb, img[ts_hdr(TS_H_MT)] = mt;
      img[ts_hdr(TS_H_NBUF)] = nbuf, img[ts_hdr(TS_H_BHI)] = bhi;
    }
#pragma unroll
    for (uint32_t i = 0; i < R; ++i) {
      img[ts_reg(TS_P_KEY, i, lid)] = pk[i], img[ts_reg(TS_P_CLOCK, i, lid)] = pc[i];
      img[ts_reg(TS_P_DOT, i, lid)] = pd[i], img[ts_reg(TS_P_ARRIVAL, i, lid)] = pa[i];
      if constexpr (MULTI) {
        img[ts_reg(TS_P_META, i, lid)] = pm[i];
        img[ts_reg(TS_P_RING_KEY, i, lid)] = sk[i], img[ts_reg(TS_P_RING_DOT, i, lid)] = sd[i];
      }
      if constexpr (SHARDS) img[ts_reg(TS_P_SHARDS, i, lid)] = pz[i];
    }
    if constexpr (MULTI && !SHARDS) img[ts_buf(0, lid)] = bk, img[ts_buf(1, lid)] = bd, img[ts_buf(2, lid)] = bc;
  }
