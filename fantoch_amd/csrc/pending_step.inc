// pending_step.inc -- what a wavefront of the pending stage does with a chunk
// of 64 order rows, lane i holding row k0 + i (its arrival row, then the rifl
// and the count at that row): the one statement of it, included into the
// anonymous namespace of pending_exec.hip (k_pending) and of
// pending_advance.hip (k_pending_advance) behind fx_pending.h and fx_wave.h.
// Where the live builders of the stream sit is a policy (below).
//
// Per chunk (pending_chunk):
//   rows of count 1   complete at once, their own head; they never see a table
//   the other rows    for every distinct rifl r (the first unserved lane's): m =
//                     ballot(rifl == r), the builder looked up once; a lane's
//                     place is the builder's got + popcount(m below it), which
//                     div / mod the count gives the command of the run it
//                     belongs to and its slot there: slot 0 creates a builder,
//                     slot count - 1 completes one, and a lane's head row is the
//                     arrival row of the nearest creator at or below it in m,
//                     else the looked-up builder's.  The looked-up builder gets
//                     its new got, or is removed, at once; a builder that is
//                     created in the chunk and still live at its end is noted
//                     in its creator's lane.  A lane whose count differs from
//                     the run's ends the run: a builder live there is the
//                     stream's count mismatch, else the lanes from it on are a
//                     run of their own, with a look-up of their own.
//   the first failing row   the lowest lane of: arrival row or count out of
//                     range, a count mismatch, (CAPPED) a creator that finds
//                     FX_PENDING_ONCHIP_LIVE builders live (the count before the
//                     chunk + creators below - completers below).  Nothing of
//                     the lanes from it on is stored or counted.
//   stores            part / head of every lane below it, index / ready of the
//                     completers (ready row: nready + completers below)
//   inserts           if no row failed, the noted builders enter the table, so
//                     at no time does it hold more than the live builders at
//                     the end of a chunk
//
// A policy states the table:
//   lookup(rr, lane)  the live builder of rifl rr: found, its place `loc`, its
//                     state word `bw` and its head row `bhead`
//   update(loc, rr, bhead, w, lane)   the looked-up builder's new state word
//   DONE              the word of a completed builder
//   insert(ir, ih, iw, lane)   a new builder; false: no place for it
//   CAPPED            a creator fails when FX_PENDING_ONCHIP_LIVE builders live

struct PendingFound {
  bool found;
  uint32_t loc, bw, bhead;
};

// ONCHIP: lane b = builder b: rifl, head row, state word (0: free).  A look-up
// is one compare and a ballot.
struct PendingRegs {
  static constexpr bool CAPPED = true;
  static constexpr uint32_t DONE = 0u;
  uint32_t rifl = 0u, head = 0u, w = 0u;

  __device__ __forceinline__ PendingFound lookup(uint32_t rr, uint32_t) const {
    PendingFound f{false, 0u, 0u, 0u};
    const uint64_t hit = __ballot(w != 0u && rifl == rr);
    if (hit) {
      f.found = true;
      f.loc = fx::ctz64(hit);
      f.bw = fx::rl(w, f.loc);
      f.bhead = fx::rl(head, f.loc);
    }
    return f;
  }
  __device__ __forceinline__ void update(uint32_t loc, uint32_t, uint32_t, uint32_t nw, uint32_t lane) {
    if (lane == loc) w = nw;
  }
  __device__ __forceinline__ bool insert(uint32_t ir, uint32_t ih, uint32_t iw, uint32_t lane) {
    const uint64_t vacant = ~__ballot(w != 0u);
    if (!vacant) return false;  // not reached: live <= FX_PENDING_ONCHIP_LIVE after a chunk that did not fail
    if (lane == fx::ctz64(vacant)) {
      rifl = ir;
      head = ih;
      w = iw;
    }
    return true;
  }
};

// HBM: `buckets` buckets of 64 entries of 16 bytes {rifl, head row, state word,
// 0}, entry i of every bucket read and written by lane i only, so a lane only
// ever reads back its own stores, in program order, and what the lanes tell
// each other goes through registers: no barrier, no atomic, every store a
// plain vector store.  A look-up is one 1 KiB load and a ballot per bucket
// walked, from the rifl's bucket on while the bucket read has no entry that
// was never used; an insert takes the lowest such entry of the first bucket
// that has one.  Completed entries stay marked and are not reused.
// CHECKED = false: a table the launch cleared itself (k_pending<true>).
// CHECKED = true: a session's table, which comes from memory the launch did
// not write: an entry counts only if its head row and its count are what a
// session writes, so no index comes from memory unchecked.
template <bool CHECKED>
struct PendingBuckets {
  static constexpr bool CAPPED = false;
  static constexpr uint32_t DONE = fx::PENDING_DONE;
  uint4* tab;
  uint32_t buckets, steps;

  __device__ __forceinline__ PendingFound lookup(uint32_t rr, uint32_t lane) const {
    PendingFound f{false, 0u, 0u, 0u};
    uint32_t bk = fx::pending_bucket(rr, buckets);
    for (uint32_t probe = 0; probe < buckets; ++probe) {
      const uint4 e = tab[bk * 64u + lane];
      const uint64_t hit =
          CHECKED ? __ballot((e.z & fx::PENDING_LIVE) != 0u && e.x == rr && e.y < steps &&
                             fx::pending_word_count(e.z) - 2u <= FX_PENDING_MAX_PARTS - 2u)
                  : __ballot((e.z & fx::PENDING_LIVE) != 0u && e.x == rr);
      if (hit) {
        const uint32_t l = fx::ctz64(hit);
        f.found = true;
        f.loc = bk * 64u + l;
        f.bw = fx::rl(e.z, l);
        f.bhead = fx::rl(e.y, l);
        break;
      }
      if (__ballot(e.z == 0u)) break;
      bk = bk + 1u == buckets ? 0u : bk + 1u;
    }
    return f;
  }
  __device__ __forceinline__ void update(uint32_t loc, uint32_t rr, uint32_t bhead, uint32_t nw, uint32_t lane) {
    if (lane == (loc & 63u)) tab[loc] = make_uint4(rr, bhead, nw, 0u);
  }
  __device__ __forceinline__ bool insert(uint32_t ir, uint32_t ih, uint32_t iw, uint32_t lane) {
    uint32_t bk = fx::pending_bucket(ir, buckets);
    for (uint32_t probe = 0; probe < buckets; ++probe) {
      const uint4 e = tab[bk * 64u + lane];
      const uint64_t unused = __ballot(e.z == 0u);
      if (unused) {
        if (lane == fx::ctz64(unused)) tab[bk * 64u + lane] = make_uint4(ir, ih, iw, 0u);
        break;
      }
      bk = bk + 1u == buckets ? 0u : bk + 1u;
    }
    return true;
  }
};

// Order rows [k0, k0 + 64) of stream s below `end`.  nready, live: the
// completed commands and the live builders so far.  False: a row failed, with
// its status in `status`, and the stream stops there.  (in, out by value: behind
// a reference the compiler no longer reads them as the kernel's arguments.)
template <class Table>
__device__ __forceinline__ bool pending_chunk(const fx_pending_batch in, const fx_pending_out out, size_t plane,
                                              uint32_t s, uint32_t k0, uint32_t end, uint32_t lane, uint64_t below,
                                              Table& tab, uint32_t& nready, uint32_t& live, uint32_t& status) {
  using fx::ctz64;
  using fx::pop64;
  using fx::rl;
  const uint32_t steps = in.steps;
  const uint32_t k = k0 + lane;
  uint32_t arow = 0u, r = 0u, c = 0u;
  bool sbad = false;
  if (k < end) {
    arow = FX_ORDER_REC(in.order[fx_index(k, s, steps)]);
    if (arow >= steps) {
      sbad = true;
    } else {
      const size_t at = fx_index(arow, s, steps);
      r = in.rifl[at];
      c = fx::pending_count(in.count[at], in.count_mask, r, in.process);
      sbad = c > FX_PENDING_MAX_PARTS;
    }
  }
  const uint64_t sfail = __ballot(sbad);
  const bool act = k < end && (sfail == 0ull || lane < ctz64(sfail));
  const bool multi = act && c > 1u;
  uint32_t head = arow, slot = 0u, ins_w = 0u;
  bool creates = false, completes = act && c == 1u, inserts = false;
  uint64_t mfail = 0ull;

  uint64_t un = __ballot(multi);
  while (un) {
    const uint32_t first = ctz64(un);
    const uint32_t rr = rl(r, first);
    uint64_t m = __ballot(multi && r == rr) & un;
    const PendingFound b = tab.lookup(rr, lane);  // the builder of rr
    const uint32_t g0 = b.found ? fx::pending_word_got(b.bw) : 0u;
    const uint32_t C = b.found ? fx::pending_word_count(b.bw) : rl(c, first);
    const uint64_t other = m & __ballot(c != C);
    if (other) {  // the run ends before the first lane of another count
      const uint32_t L = ctz64(other);
      const uint64_t run = m & ((1ull << L) - 1ull);
      if ((g0 + pop64(run)) % C != 0u) {  // a builder of count C is live at lane L
        mfail |= 1ull << L;
        un &= ~m;
      }
      m = run;
    }
    un &= ~m;
    const uint32_t total = g0 + pop64(m);
    const bool mine = (m >> lane) & 1ull;
    const uint32_t p = g0 + pop64(m & below);
    uint32_t q = 0u, sl = p, rem = total == C ? 0u : total;
    if (total > C) {
      q = p / C;
      sl = p - q * C;
      rem = total % C;
    }
    const bool cr = mine && sl == 0u;
    const uint64_t crs = __ballot(cr) & (below | (1ull << lane));
    // every lane takes part in the exchange
    const uint32_t from = (uint32_t)__shfl((int)arow, (int)(crs ? 63u - (uint32_t)__builtin_clzll(crs) : lane));
    if (mine) {
      head = crs ? from : b.bhead;
      slot = sl;
      creates = cr;
      completes = sl == C - 1u;
      // the builder created in this chunk that outlives it
      if (rem != 0u && (!b.found || total > C) && p == total - rem) {
        inserts = true;
        ins_w = fx::pending_word(C, rem);
      }
    }
    if (b.found) tab.update(b.loc, rr, b.bhead, total >= C ? Table::DONE : fx::pending_word(C, total), lane);
  }

  const uint64_t crs = __ballot(creates), cps = __ballot(completes && c > 1u), fin = __ballot(completes);
  uint64_t cfail = 0ull;
  if (Table::CAPPED)
    cfail = __ballot(creates && live + pop64(crs & below) - pop64(cps & below) >= FX_PENDING_ONCHIP_LIVE);
  const uint64_t fail = sfail | mfail | cfail;
  const uint64_t ok = fail ? (1ull << ctz64(fail)) - 1ull : ~0ull;
  if (act && ((ok >> lane) & 1ull)) {
    const size_t at = fx_index(arow, s, steps);
    if (c == 0u) {
      out.head[at] = FX_PENDING_IGNORED;
    } else {
      const size_t hat = fx_index(head, s, steps);
      out.part[slot * plane + hat] = arow;
      out.head[at] = head;
      if (completes) {
        const uint32_t i = nready + pop64(fin & below);
        out.index[hat] = i;
        out.ready[fx_index(i, s, steps)] = head;
      }
    }
  }
  nready += pop64(fin & ok);
  live += pop64(crs & ok) - pop64(cps & ok);
  if (fail) {
    status = (cfail >> ctz64(fail)) & 1ull ? FX_ERR_CAPACITY : FX_ERR_INVALID_ARG;
    return false;
  }

  uint64_t ins = __ballot(inserts);
  while (ins) {
    const uint32_t l = ctz64(ins);
    ins &= ins - 1ull;
    if (!tab.insert(rl(r, l), rl(arow, l), rl(ins_w, l), lane)) break;
  }
  return true;
}
