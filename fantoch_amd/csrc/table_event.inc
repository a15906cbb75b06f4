// table_event.inc -- one own event of a table executor stream: the body of
// k_table's event loop (table_exec.hip), included where that loop handles input
// row r as handled row hj of the stream (hj == r but in a group, where the
// messages from other shards take rows of their own).  The tile row holding
// row r is in `row`.  FX_EVENT_NEXT leaves to the next event, FX_EVENT_STOP
// leaves with the stream stopped (err is set): `continue` and `break` of the
// loop, or the returns of the callable unit the group kernel needs, whose
// round loop no event may leave.
    const uint32_t kq = r & 3u;
    const size_t at = fx_index(r, s, a.steps);
    const size_t oat = fx_index(hj, s, osteps);
    const uint32_t h = rl(row, kq);
    const uint32_t k = FX_TABLE_HDR_KEY(h), nv = FX_TABLE_HDR_NVOTES(h);
    if constexpr (SHARDS && !GROUP) {
      if (h >> 24 == FX_TABLE_HDR_STABLE(0) >> 24) {  // StableAtShard from another shard (:140-142)
        if (k >= keys) { err = FX_ERR_INVALID_ARG; FX_EVENT_STOP; }
        const uint32_t d = rl(row, 4u + kq);
        if (FX_DOT_SRC(d) < 1 || FX_DOT_SRC(d) > n || FX_DOT_SEQ(d) == 0) { err = FX_ERR_DOT_RANGE; FX_EVENT_STOP; }
        if (!at_commit) stable_msg(k, d);
        if (err) FX_EVENT_STOP;
        FX_EVENT_NEXT;  // (the drain comes before the next event, or after the last)
      }
    }
    if (nv > a.vmax || k >= keys) { err = FX_ERR_INVALID_ARG; FX_EVENT_STOP; }
    if (FX_TABLE_HDR_KIND(h) == FX_TABLE_ATTACHED) {
      const uint32_t d = rl(row, 4u + kq), c = rl(row, 8u + kq);
      const uint32_t src = FX_DOT_SRC(d);
      uint32_t K = 1, SH = 1;
      (void)K;
      (void)SH;
      if constexpr (MULTI) {
        K = rl(row, 60u + kq);
        if constexpr (SHARDS) {  // FX_TABLE_PS_WORD(nkeys, shards)
          SH = K >> 8;
          K &= 0xFFu;
          if (SH < 1 || SH > FX_TABLE_MAX_CMD_SHARDS) { err = FX_ERR_INVALID_ARG; FX_EVENT_STOP; }
        }
        if (K < 1 || K > FX_TABLE_MAX_CMD_KEYS) { err = FX_ERR_INVALID_ARG; FX_EVENT_STOP; }
      }
      if (src < 1 || src > n || FX_DOT_SEQ(d) == 0) { err = FX_ERR_DOT_RANGE; FX_EVENT_STOP; }
      if (at_commit) {  // executor.rs:125-126
        if (lid == 0) {
          a.order[fx_index(nexec, s, osteps)] = hj | FX_ORDER_SCC_START;
          a.release[oat] = hj;
        }
        ++nexec;
        FX_EVENT_NEXT;
      }
      // ops.insert(sort_id, pending) must find the slot free (mod.rs:163-165)
      uint64_t dup = 0;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i)
        dup |= __ballot(pk[i] == k && pc[i] == c && pd[i] == d && (!MULTI || m_state(pm[i]) == ST_TABLE));
      if (dup) { err = FX_ERR_DOUBLE_INDEX; FX_EVENT_STOP; }
      if constexpr (MULTI) {
        // the input contract, against the command's ops that have not executed:
        // same nkeys (and shards) and clock, another key, fewer than nkeys, none told
        uint64_t bad = 0;
        uint32_t mates = 0;
#pragma unroll
        for (uint32_t i = 0; i < R; ++i) {
          const bool m = pk[i] != NONE && pd[i] == d;
          mates += (uint32_t)__builtin_popcountll(__ballot(m));
          bad |= __ballot(m && (pk[i] == k || pc[i] != c || m_nkeys(pm[i]) != K || m_state(pm[i]) == ST_TOLD ||
                                (SHARDS && (pz[i] >> 8) != SH)));
        }
        if (bad || mates >= K) { err = FX_ERR_INVALID_ARG; FX_EVENT_STOP; }
      }
      bool placed = false;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i) {
        if (!placed) {
          const uint64_t fr = __ballot(pk[i] == NONE);
          if (fr) {
            if (lid == (uint32_t)__builtin_ctzll(fr)) {
              pk[i] = k, pc[i] = c, pd[i] = d, pa[i] = hj;
              if constexpr (MULTI) pm[i] = (K - 1u) << 28;
              if constexpr (SHARDS) pz[i] = SH | (SH << 8);
            }
            placed = true;
          }
        }
      }
      if (!placed) { err = FX_ERR_CAPACITY; FX_EVENT_STOP; }
    } else if (at_commit) {
      FX_EVENT_NEXT;  // executor.rs:134-139: votes are ignored
    }

    // add_detached_votes (mod.rs:171-194): the ranges in order, each on the
    // lane of its voter
    uint32_t f = 0, w = 0;
    if (vlane) {
      if constexpr (HBM) {
        f = g[(size_t)k * NV + lid];
      } else {
        f = smem[lb + k * 32u + lid];
        w = smem[lb + k * 32u + 16u + lid];
      }
    }
    uint32_t fail = 0;
    for (uint32_t j = 0; j < nv; ++j) {
      uint32_t voter, st, en;
      if (j < 4u) {
        voter = rl(row, 4u * (3u + 3u * j) + kq);
        st = rl(row, 4u * (4u + 3u * j) + kq);
        en = rl(row, 4u * (5u + 3u * j) + kq);
      } else {
        const uint32_t* vp = a.votes + (size_t)(3u * j) * a.plane + at;
        voter = (uint32_t)__builtin_amdgcn_readfirstlane((int)vp[0]);
        st = (uint32_t)__builtin_amdgcn_readfirstlane((int)vp[a.plane]);
        en = (uint32_t)__builtin_amdgcn_readfirstlane((int)vp[2 * a.plane]);
      }
      if (voter - 1u >= n || st == 0 || st > en) { fail = FX_ERR_VOTE_RANGE; break; }
      uint32_t lf = 0;
      if (lid == voter - 1u) {
        // table_window.h; HBM: word i of this voter's ring at win[i * NV]
        if constexpr (HBM) lf = add_range_ring<!SHARDS>(f, g + ((size_t)keys + (size_t)k * WB) * NV + lid, NV, st, en);
        else lf = add_range_word<MULTI>(f, w, st, en);
      }
      fail = rl(lf, voter - 1u);
      if (fail) break;
    }
    if (fail) { err = fail; FX_EVENT_STOP; }
    if (vlane) {
      if constexpr (HBM) {
        g[(size_t)k * NV + lid] = f;
      } else {
        smem[lb + k * 32u + lid] = f;
        smem[lb + k * 32u + 16u + lid] = w;
      }
    }

    // stable_ops (mod.rs:196-240)
    uint64_t onkey = 0;
#pragma unroll
    for (uint32_t i = 0; i < R; ++i) onkey |= __ballot(pk[i] == k && (!MULTI || m_state(pm[i]) == ST_TABLE));
    if (!onkey) FX_EVENT_NEXT;
    const uint32_t stable = stable_of(f, n, a.thr, lid);
    bool sel[R];
    uint64_t sb[R];
    uint32_t rank[R], total = 0;
#pragma unroll
    for (uint32_t i = 0; i < R; ++i) {
      sel[i] = pk[i] == k && pc[i] <= stable && (!MULTI || m_state(pm[i]) == ST_TABLE);
      sb[i] = __ballot(sel[i]);
      rank[i] = 0;
      total += (uint32_t)__builtin_popcountll(sb[i]);
    }
    if (!total) FX_EVENT_NEXT;
#pragma unroll
    for (uint32_t i2 = 0; i2 < R; ++i2) {
      for (uint64_t b = sb[i2]; b; b &= b - 1u) {
        const uint32_t l = (uint32_t)__builtin_ctzll(b);
        const uint32_t oc = rl(pc[i2], l), od = rl(pd[i2], l);
#pragma unroll
        for (uint32_t i = 0; i < R; ++i) rank[i] += (oc < pc[i] || (oc == pc[i] && od < pd[i])) ? 1u : 0u;
      }
    }
    if constexpr (MULTI) {
      // send_stable_or_execute (executor.rs:237-277).  With the key's queue
      // empty and single-key ops only, all execute at once; otherwise the
      // ops join the queue in their order and, if it was empty, are tried
      // from its head until one is handed back.
      uint64_t queued = 0, multi = 0;
#pragma unroll
      for (uint32_t i = 0; i < R; ++i) {
        queued |= __ballot(pk[i] == k && m_state(pm[i]) != ST_TABLE);
        multi |= __ballot(sel[i] && (m_nkeys(pm[i]) != 1u || (SHARDS && (pz[i] >> 8) != 1u)));
      }
      if (queued || multi) {
#pragma unroll
        for (uint32_t i = 0; i < R; ++i)
          if (sel[i]) pm[i] = (pm[i] & ~(SEQ_MASK | (3u << 26))) | (ST_QUEUED << 26) | (qseq + rank[i]);
        qseq += total;
        if (!queued) run_queue(k);
        FX_EVENT_NEXT;
      }
    }
#pragma unroll
    for (uint32_t i = 0; i < R; ++i) {
      if (sel[i]) {
        a.order[fx_index(nexec + rank[i], s, osteps)] = pa[i] | FX_ORDER_SCC_START;
        a.release[fx_index(pa[i], s, osteps)] = hj;
        pk[i] = NONE;
      }
    }
    nexec += total;
