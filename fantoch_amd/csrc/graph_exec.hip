// graph_exec.hip — the lane-per-stream slot tiers of the batched GraphExecutor
// (FX_TIER_LDS_LARGE, FX_TIER_GLOBAL, FX_TIER_LANE) for gfx950 (MI355X): the
// tier layouts (Tier), the executor (Exec), the kernel (k_graph_exec) and the
// tiers' face towards the tier table (graph_tiers.hip): SlotTier<FX_TIER_*>.
//
// One lane = one commit stream = one (instance, process) executor of the
// reference (fantoch_ps/src/executor/graph/executor.rs:19-29 owns one
// DependencyGraph each).  A 64-thread workgroup is one wavefront running 64
// independent executors; there is no inter-lane communication, so nothing
// here depends on dispatch order or XCD placement.
//
// State restates the reference's containers as fixed tables (SURVEY §8(a)
// rows a4-a10):
//   executed clock AEClock (threshold 0.9.1; tarjan.rs:131-132,293):
//     per source a u32 frontier + an XW-word bitmap of executed seqs above it
//   VertexIndex (index.rs:18-51): P pending-vertex slots {dot, rec, wait,
//     tarjan id/low/visited-epoch, cached deps}
//   PendingIndex (index.rs:145-208): slot.wait = the missing dot the vertex is
//     registered on (a vertex is registered on at most one dot at a time)
//   TarjanSCCFinder (tarjan.rs:25-33): explicit DFS frame stack + Tarjan stack
//   check_pending's `dots` (mod.rs:556-587): LIFO worklist
// Every field lives in memory, in a lane-interleaved layout: word w of lane l
// at dword (w * 64 + l), so whatever slot a lane touches the LDS bank is
// (l mod 32) — conflict-free.  FX_TIER_LANE and FX_TIER_LDS_LARGE keep the
// words in LDS, FX_TIER_GLOBAL in HBM (its `state` block).
//
// Divergence: the slow path (Tarjan search, check_pending, try_pending) is a
// flat state machine — every iteration each lane performs ONE micro-op (one
// DFS edge or frame pop, one waiter pick, one worklist pop) — so a wavefront's
// cost per Add is the max over its lanes of their micro-op counts instead of
// the product of nested divergent loop trip counts.
//
// Records stream through a double-buffered register pipeline (a block = 4
// steps = one 16-byte load per lane per plane, see fx_index in fantoch_amd.h)
// whose loads have a static count, so waits are precise vmcnt(N).  Within a
// block lanes advance through their 4 steps independently.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fantoch_amd.h"
#include "fx_internal.h"

namespace fx {

constexpr uint32_t WAVE = 64;

template <uint32_t NSRC_, uint32_t P_, uint32_t XW_, uint32_t C_, bool GLOBAL_>
struct Tier {
  static constexpr uint32_t NSRC = NSRC_;  // sources (processes) supported
  static constexpr uint32_t P = P_;        // pending-vertex slots
  static constexpr uint32_t XW = XW_;      // clock window words per source
  static constexpr uint32_t C = C_;        // cached not-yet-executed deps per vertex
  static constexpr bool GLOBAL = GLOBAL_;  // state in HBM instead of LDS
  static constexpr bool SMALL = P <= 15;   // u16 tarjan words, slot hints in cached deps
  using Mask = typename std::conditional<(P <= 32), uint32_t, uint64_t>::type;
  // words per lane
  static constexpr uint32_t CLKS = 1 + XW;
  static constexpr uint32_t CLK = 0;
  static constexpr uint32_t DOT = CLK + NSRC * CLKS;
  static constexpr uint32_t WAIT = DOT + P;
  static constexpr uint32_t REC = WAIT + P;  // arrival index | ncached << 26
  static constexpr uint32_t TL = REC + P;    // tarjan id | low | visited epoch
  static constexpr uint32_t DEP = TL + (SMALL ? (P + 1) / 2 : P);  // [C][P] dot | hint << 28
  static constexpr uint32_t TS = DEP + C * P;        // Tarjan stack, u8 slots
  static constexpr uint32_t FR = TS + (P + 3) / 4;   // DFS parent frames, u16 slot | dep idx << 8
  static constexpr uint32_t WL = FR + (P + 1) / 2;   // worklist, P + 1 packed dots
  static constexpr uint32_t MEM = WL + P + 1;        // words in LDS (or HBM)
  static constexpr uint32_t WORDS = MEM + 6;  // + occ(2) wmask(2) k err|epoch
  static_assert(P <= 64, "slot masks are at most u64");
  static_assert(P < 256, "slots are u8");
  static_assert(C < 32, "ncached is 5 bits");
};

// LDS bytes / wave: TierLane 35,840 -> 4 waves / CU;
// Tier1 123,136 -> 1 wave / CU.
using TierLane = Tier<8, 12, 1, 5, false>;
using Tier1 = Tier<8, 32, 4, 8, false>;
using Tier2 = Tier<8, 64, 32, 16, true>;  // HBM-resident, 1024-bit clock windows


__device__ __forceinline__ uint32_t hdr_nd(uint32_t h) { return (h >> 24) & 31u; }

// Picks among registers by a per-lane value.  Arithmetic masks instead of
// selects: LLVM folds `i == k ? a[k] : r` chains back into a dynamically
// indexed load, which demotes the registers (and the executor) to scratch.
__device__ __forceinline__ uint32_t lmask(bool c) { return 0u - (uint32_t)c; }

enum : uint32_t { PH_IDLE = 0, PH_DFS = 1, PH_TRY = 2, PH_CHECK = 3 };

template <class T, uint32_t DCAP>
struct Exec {
  using Mask = typename T::Mask;
  static constexpr Mask ONE = 1;

  uint32_t* st;  // this lane's memory state: word w at st[w * WAVE]
  Mask occ = 0, wmask = 0, tmask = 0;
  uint32_t k = 0, err = 0, epoch = 1, nwl = 0, cur = 0;
  uint32_t stream = 0, n = 0, steps = 0, dmax = 0;
  size_t plane = 0;
  const uint32_t* deps = nullptr;
  uint32_t* order = nullptr;
  uint32_t* release = nullptr;
  // find_scc context
  uint32_t phase = PH_IDLE, root = 0, idc = 0, nts = 0, nfr = 0, missing = 0;
  uint32_t fv = 0, fdi = 0, fnc = 0;
  bool in_try = false, emitted = false;

  __device__ __forceinline__ uint32_t& w(uint32_t i) { return st[i * WAVE]; }
  __device__ __forceinline__ uint8_t& ts(uint32_t i) {
    return reinterpret_cast<uint8_t*>(&w(T::TS + (i >> 2)))[i & 3];
  }
  __device__ __forceinline__ uint16_t& fr(uint32_t i) {
    return reinterpret_cast<uint16_t*>(&w(T::FR + (i >> 1)))[i & 1];
  }
  __device__ __forceinline__ uint32_t& wl(uint32_t i) { return w(T::WL + i); }
  __device__ __forceinline__ size_t at(uint32_t step) const { return fx_index(step, stream, steps); }

  // ------------------------------------------------------- slot fields
  __device__ __forceinline__ uint32_t dot_of(uint32_t sl) {
    return w(T::DOT + sl);
  }
  __device__ __forceinline__ void set_dot(uint32_t sl, uint32_t v) {
    w(T::DOT + sl) = v;
  }
  __device__ __forceinline__ uint32_t wait_of(uint32_t sl) {
    return w(T::WAIT + sl);
  }
  __device__ __forceinline__ void set_wait(uint32_t sl, uint32_t v) {
    w(T::WAIT + sl) = v;
  }
  __device__ __forceinline__ uint32_t rec_of(uint32_t sl) {
    return w(T::REC + sl);
  }
  __device__ __forceinline__ void set_rec(uint32_t sl, uint32_t v) {
    w(T::REC + sl) = v;
  }
  // Tarjan word: id | low | visited epoch (u16 4|4|8 on small tiers, u32 12|12|8)
  static constexpr uint32_t IDB = T::SMALL ? 4 : 12;
  static constexpr uint32_t IDM = (1u << IDB) - 1;
  __device__ __forceinline__ uint32_t tl_of(uint32_t sl) {
    if constexpr (T::SMALL) return reinterpret_cast<uint16_t*>(&w(T::TL + (sl >> 1)))[sl & 1];
    else return w(T::TL + sl);
  }
  __device__ __forceinline__ void set_tl(uint32_t sl, uint32_t v) {
    if constexpr (T::SMALL) reinterpret_cast<uint16_t*>(&w(T::TL + (sl >> 1)))[sl & 1] = (uint16_t)v;
    else w(T::TL + sl) = v;
  }
  static __device__ __forceinline__ uint32_t tid(uint32_t t) { return t & IDM; }
  static __device__ __forceinline__ uint32_t tlow(uint32_t t) { return (t >> IDB) & IDM; }
  static __device__ __forceinline__ uint32_t tep(uint32_t t) { return t >> (2 * IDB); }
  static __device__ __forceinline__ uint32_t tmk(uint32_t id, uint32_t low, uint32_t ep) {
    return id | (low << IDB) | (ep << (2 * IDB));
  }

  // ---------------------------------------------- executed clock (AEClock)
  // AEClock::contains (tarjan.rs:131-132)
  __device__ __forceinline__ bool clk_contains(uint32_t d) {
    const uint32_t si = (d >> FX_SEQ_BITS) - 1u;
    if (si >= n) return false;
    const uint32_t seq = d & FX_SEQ_MASK;
    const uint32_t b = T::CLK + si * T::CLKS;
    const uint32_t f = w(b);
    if (seq <= f) return true;
    const uint32_t off = seq - f - 1u;
    if (off >= 32u * T::XW) return false;
    return (w(b + 1 + (off >> 5)) >> (off & 31u)) & 1u;
  }
  // AEClock::add (tarjan.rs:293): frontier + exception window
  __device__ __forceinline__ void clk_add(uint32_t d) {
    const uint32_t si = (d >> FX_SEQ_BITS) - 1u;
    if (si >= n) { err = FX_ERR_DOT_RANGE; return; }
    const uint32_t seq = d & FX_SEQ_MASK;
    const uint32_t b = T::CLK + si * T::CLKS;
    const uint32_t f = w(b);
    if (seq <= f) return;
    const uint32_t off = seq - f - 1u;
    if (off >= 32u * T::XW) { err = FX_ERR_CAPACITY; return; }
    if (off != 0) {
      w(b + 1 + (off >> 5)) |= 1u << (off & 31u);
      return;
    }
    uint32_t t = 1;  // 1 + trailing ones of the window from bit 1
    while (t < 32u * T::XW) {
      const uint32_t word = w(b + 1 + (t >> 5)) >> (t & 31u);
      const uint32_t avail = 32u - (t & 31u);
      const uint32_t inv = ~word;
      const uint32_t run = inv ? (uint32_t)__builtin_ctz(inv) : 32u;
      const uint32_t r = run < avail ? run : avail;
      t += r;
      if (r < avail) break;
    }
    w(b) = f + t;
    const uint32_t ws = t >> 5, sh = t & 31u;
#pragma unroll
    for (uint32_t q = 0; q < T::XW; ++q) {
      const uint32_t lo = q + ws;
      uint32_t v = lo < T::XW ? (w(b + 1 + lo) >> sh) : 0u;
      if (sh && lo + 1 < T::XW) v |= w(b + 2 + lo) << (32u - sh);
      w(b + 1 + q) = v;
    }
  }

  // ----------------------------------------------- VertexIndex slot table
  __device__ __forceinline__ int pt_find(uint32_t d) {
    for (Mask m = occ; m; m &= m - 1) {
      const int sl = __builtin_ctzll((uint64_t)m);
      if (w(T::DOT + sl) == d) return sl;
    }
    return -1;
  }
  // registered waiters of x: PendingIndex::remove(x) (index.rs:205-207)
  __device__ __forceinline__ Mask waiters(uint32_t x) {
    Mask t = 0;
    for (Mask m = wmask; m; m &= m - 1) {
      const int sl = __builtin_ctzll((uint64_t)m);
      if (w(T::WAIT + sl) == x) t |= ONE << sl;
    }
    return t;
  }
  // slot with the smallest dot among `m` (canonical C2 order)
  __device__ __forceinline__ int argmin_dot(Mask m) {
    int best = -1;
    uint32_t bd = 0xFFFFFFFFu;
    for (; m; m &= m - 1) {
      const int sl = __builtin_ctzll((uint64_t)m);
      const uint32_t dd = w(T::DOT + sl);
      if (dd < bd) { bd = dd; best = sl; }
    }
    return best;
  }
  __device__ __forceinline__ int pt_insert(uint32_t d, uint32_t rec) {
    constexpr Mask full = T::P == 8 * sizeof(Mask) ? ~(Mask)0 : ((ONE << T::P) - 1);
    const Mask fre = ~occ & full;
    if (!fre) { err = FX_ERR_CAPACITY; return -1; }
    const uint32_t sl = __builtin_ctzll((uint64_t)fre);
    occ |= ONE << sl;
    set_dot(sl, d);
    set_rec(sl, rec);
    set_wait(sl, 0);
    set_tl(sl, 0);
    return (int)sl;
  }
  __device__ __forceinline__ void pt_free(uint32_t sl) {
    const Mask keep = ~(ONE << sl);
    occ &= keep;
    wmask &= keep;
    tmask &= keep;
  }
  // Vertex::deps restricted to the deps not executed at insertion (executed
  // deps are ignored by every later search, tarjan.rs:128-145, and the
  // executed clock only grows), ascending; a dep pending at insertion carries
  // its slot + 1 (it can only leave that slot by being executed).
  __device__ __forceinline__ void pt_cache_dep(uint32_t sl, uint32_t d, uint32_t dep, uint32_t& nc) {
    if (dep == d || clk_contains(dep)) return;
    if ((dep >> FX_SEQ_BITS) > 15u) { err = FX_ERR_DOT_RANGE; return; }
    if (nc >= T::C) { err = FX_ERR_CAPACITY; return; }
    uint32_t hint = 0;
    if constexpr (T::SMALL) hint = (uint32_t)(pt_find(dep) + 1);
    w(T::DEP + nc * T::P + sl) = dep | (hint << 28);
    ++nc;
  }
  // VertexIndex::index(Vertex::new(dot, cmd, deps, time)) (index.rs:33-37):
  // deps j < DCAP come from the prefetched registers, the rest from HBM.
  __device__ __forceinline__ int insert_vertex(uint32_t i, uint32_t d, uint32_t nd, const uint32_t* rdeps) {
    const int sl = pt_insert(d, i);
    if (sl < 0) return -1;
    uint32_t nc = 0;
#pragma unroll
    for (uint32_t j = 0; j < DCAP; ++j)
      if (j < nd) pt_cache_dep((uint32_t)sl, d, rdeps[j], nc);
    for (uint32_t j = DCAP; j < nd; ++j) pt_cache_dep((uint32_t)sl, d, deps[(size_t)j * plane + at(i)], nc);
    if (err) return -1;
    set_rec((uint32_t)sl, i | (nc << 26));
    return sl;
  }

  // try_pending's `visited` set (mod.rs:598): an epoch stamp per slot
  __device__ __forceinline__ void new_epoch() {
    epoch = (epoch + 1) & 0xFFu;
    if (epoch == 0) {
      for (Mask m = occ; m; m &= m - 1) {
        const uint32_t sl = __builtin_ctzll((uint64_t)m);
        const uint32_t t = tl_of(sl);
        set_tl(sl, tmk(tid(t), tlow(t), 0));
      }
      epoch = 1;
    }
  }

  // save_scc (mod.rs:488-523) for one member: to_execute + executed clock
  __device__ __forceinline__ void emit(uint32_t rec, uint32_t d, bool start) {
    if (k >= steps) { err = FX_ERR_ORDER_OVERFLOW; return; }
    order[at(k)] = rec | (start ? FX_ORDER_SCC_START : 0u);
    release[at(rec)] = cur;
    ++k;
    clk_add(d);
  }

  // ------------------------------ find_scc as a micro-op state machine
  // find_scc (mod.rs:409-486) = TarjanSCCFinder::strong_connect
  // (tarjan.rs:96-316) run iteratively + save_scc + finalize (tarjan.rs:60-93)
  __device__ __forceinline__ void dfs_start(uint32_t r, bool intry) {
    root = r;
    in_try = intry;
    emitted = false;
    missing = 0;
    idc = 1;
    set_tl(r, tmk(1, 1, tep(tl_of(r))));
    ts(0) = (uint8_t)r;
    nts = 1;
    nfr = 0;
    fv = r;
    fdi = 0;
    fnc = rec_of(r) >> 26;
    phase = PH_DFS;
  }

  // SCC rooted at fv: members are TS[pos..nts), saved in ascending dot order
  // (SCC = BTreeSet<Dot>, tarjan.rs:15); executed clock updated per member.
  __device__ __forceinline__ void save_scc() {
    uint32_t pos = nts - 1;
    while (ts(pos) != fv) --pos;
    for (uint32_t a = pos + 1; a < nts; ++a) {
      const uint8_t key = ts(a);
      const uint32_t kd = dot_of(key);
      uint32_t b = a;
      while (b > pos && dot_of(ts(b - 1)) > kd) {
        ts(b) = ts(b - 1);
        --b;
      }
      ts(b) = key;
    }
    for (uint32_t a = pos; a < nts; ++a) {
      const uint32_t sl = ts(a);
      const uint32_t d = dot_of(sl);
      emit(rec_of(sl) & 0x03FFFFFFu, d, a == pos);
      wl(nwl++) = d;
      pt_free(sl);
    }
    nts = pos;
    emitted = true;
  }

  __device__ __forceinline__ void dfs_finish() {
    // finalize: reset ids of the vertices left on the stack; in try_pending a
    // failed search that saved no SCC adds them to `visited` (mod.rs:621-629)
    const bool mark = in_try && missing != 0 && !emitted;
    for (uint32_t a = 0; a < nts; ++a) {
      const uint32_t sl = ts(a);
      set_tl(sl, tmk(0, 0, mark ? epoch : tep(tl_of(sl))));
    }
    nts = 0;
    if (missing) {  // index_pending(dot, missing) (mod.rs:525-554)
      set_wait(root, missing);
      wmask |= ONE << root;
    }
    if (in_try) {
      if (!missing || emitted) new_epoch();  // visited.clear() (mod.rs:607, 621-623)
      phase = PH_TRY;
    } else {
      phase = PH_CHECK;
    }
  }

  // one DFS edge or one frame pop
  __device__ __forceinline__ void dfs_iter() {
    if (fdi < fnc) {
      const uint32_t cwd = w(T::DEP + fdi * T::P + fv);
      ++fdi;
      const uint32_t dep = cwd & 0x0FFFFFFFu;
      if (clk_contains(dep)) return;  // executed (tarjan.rs:128-145)
      int x = -1;
      if constexpr (T::SMALL) {
        const uint32_t h = cwd >> 28;
        if (h) x = (int)h - 1;
      }
      if (x < 0) x = pt_find(dep);
      if (x < 0) {  // missing: give up (tarjan.rs:148-157, shard_count == 1)
        missing = dep;
        dfs_finish();
        return;
      }
      const uint32_t tx = tl_of((uint32_t)x);
      if (tid(tx) == 0) {  // not visited: recurse (tarjan.rs:172-214)
        ++idc;
        set_tl((uint32_t)x, tmk(idc, idc, tep(tx)));
        ts(nts++) = (uint8_t)x;
        fr(nfr++) = (uint16_t)(fv | (fdi << 8));
        fv = (uint32_t)x;
        fdi = 0;
        fnc = rec_of(fv) >> 26;
      } else {  // visited and on the stack (tarjan.rs:215-225)
        const uint32_t tv = tl_of(fv);
        if (tid(tx) < tlow(tv)) set_tl(fv, tmk(tid(tv), tid(tx), tep(tv)));
      }
    } else {
      const uint32_t tv = tl_of(fv);
      const uint32_t lowv = tlow(tv);
      if (tid(tv) == lowv) {  // SCC root (tarjan.rs:233-312)
        save_scc();
        if (err) { phase = PH_IDLE; return; }
      }
      if (nfr == 0) {  // root done: Found
        dfs_finish();
        return;
      }
      const uint32_t f = fr(--nfr);  // back in the parent: low = min(low, dep.low) (tarjan.rs:211)
      fv = f & 0xFFu;
      fdi = f >> 8;
      fnc = rec_of(fv) >> 26;
      const uint32_t tp = tl_of(fv);
      if (lowv < tlow(tp)) set_tl(fv, tmk(tid(tp), lowv, tep(tp)));
    }
  }

  // try_pending (mod.rs:589-642): next waiter of the snapshot, ascending (C2)
  __device__ __forceinline__ void try_iter() {
    if (!tmask) { phase = PH_CHECK; return; }
    const int best = argmin_dot(tmask);
    tmask &= ~(ONE << best);
    if (tep(tl_of((uint32_t)best)) == epoch) return;  // visited: skipped, not re-registered
    dfs_start((uint32_t)best, true);
  }

  // check_pending (mod.rs:556-587): pop one released dot (LIFO)
  __device__ __forceinline__ void check_iter() {
    if (nwl == 0 || !wmask) {
      nwl = 0;
      phase = PH_IDLE;
      return;
    }
    const uint32_t x = wl(--nwl);
    const Mask t = waiters(x);
    if (!t) return;
    wmask &= ~t;  // PendingIndex::remove(x): the waiters are no longer registered
    tmask = t;
    new_epoch();  // try_pending's fresh `visited`
    phase = PH_TRY;
  }

  __device__ __forceinline__ void slow_iter() {
    if (phase == PH_DFS) dfs_iter();
    if (phase == PH_TRY) try_iter();
    if (phase == PH_CHECK) check_iter();
    if (err) phase = PH_IDLE;
  }

  // GraphExecutor::handle(Add) (executor.rs:69-80) -> handle_add (mod.rs:213-275):
  // the fast path completes here; otherwise the lane enters the state machine.
  __device__ __forceinline__ void step_start(uint32_t i, uint32_t d, uint32_t h, const uint32_t* rdeps,
                                             bool at_commit) {
    cur = i;
    nwl = 0;
    const uint32_t nd = hdr_nd(h), kind = h >> 29;
    if (nd > dmax) { err = FX_ERR_INVALID_ARG; return; }  // deps beyond the dep planes
    if ((d >> FX_SEQ_BITS) - 1u >= n || (d & FX_SEQ_MASK) == 0) { err = FX_ERR_DOT_RANGE; return; }
    if (at_commit) {  // execute_at_commit bypass (executor.rs:72-73)
      order[at(k)] = i | FX_ORDER_SCC_START;
      release[at(i)] = i;
      ++k;
      return;
    }
    if (occ && pt_find(d) >= 0) { err = FX_ERR_DOUBLE_INDEX; return; }  // mod.rs:233-237
    if (kind == FX_KIND_INDEX_ONLY) {
      insert_vertex(i, d, nd, rdeps);
      return;
    }
    // Fast path: every dep is self or executed -> strong_connect visits only
    // the new vertex and saves it as a singleton SCC.
    bool fast = nd <= DCAP;
    uint32_t prev = 0;
#pragma unroll
    for (uint32_t j = 0; j < DCAP; ++j) {
      if (j < nd) {
        const uint32_t dep = rdeps[j];
        if (dep <= prev) err = FX_ERR_DEPS_UNSORTED;
        prev = dep;
        if (dep != d && !clk_contains(dep)) fast = false;
      }
    }
    if (err) return;
    if (fast) {
      emit(i, d, true);
      if (wmask && !err) {  // check_pending([dot])
        wl(0) = d;
        nwl = 1;
        phase = PH_CHECK;
      }
    } else {
      const int sl = insert_vertex(i, d, nd, rdeps);
      if (sl >= 0) dfs_start((uint32_t)sl, false);
    }
  }
};

template <class T, uint32_t DCAP>
__global__ __launch_bounds__(64) void k_graph_exec(KArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const uint32_t lane = threadIdx.x;
  const uint32_t gl = blockIdx.x * WAVE + lane;
  const bool active = gl < a.num_lanes;
  const uint32_t s = active ? (a.stream_map ? a.stream_map[gl] : gl) : 0u;
  const uint32_t len = active ? (a.lengths ? min(a.lengths[s], a.steps) : a.steps) : 0u;
  uint32_t* gblock = a.state ? a.state + (size_t)blockIdx.x * T::WORDS * WAVE : nullptr;

  Exec<T, DCAP> e;
  if constexpr (T::GLOBAL) e.st = gblock + lane;
  else e.st = smem + lane;
  e.stream = s;
  e.n = a.n;
  e.steps = a.steps;
  e.plane = a.plane;
  e.dmax = a.dmax;
  e.deps = a.deps;
  e.order = a.order;
  e.release = a.release;

  if (a.flags & FX_FLAG_INIT) {
    for (uint32_t q = 0; q < T::NSRC * T::CLKS; ++q) e.w(T::CLK + q) = 0;
    if (a.init_frontier && active) {
#pragma unroll
      for (uint32_t p = 0; p < T::NSRC && p < 8; ++p) {
        e.w(T::CLK + p * T::CLKS) = a.init_frontier[(size_t)s * 8 + p];
      }
    }
  } else {
    if constexpr (!T::GLOBAL) {
      for (uint32_t q = 0; q < T::MEM; ++q) smem[q * WAVE + lane] = gblock[q * WAVE + lane];
    }
    const uint32_t* r = gblock + (size_t)T::MEM * WAVE + lane;
    e.occ = (typename T::Mask)((uint64_t)r[0] | ((uint64_t)r[WAVE] << 32));
    e.wmask = (typename T::Mask)((uint64_t)r[2 * WAVE] | ((uint64_t)r[3 * WAVE] << 32));
    e.k = r[4 * WAVE];
    e.err = r[5 * WAVE] & 0xFFFFu;
    e.epoch = r[5 * WAVE] >> 16;
  }
  if (!active) e.err = FX_ERR_INVALID_ARG;  // idle lane (its loads read stream 0)

  const bool at_commit = (a.flags & FX_FLAG_EXECUTE_AT_COMMIT) != 0;
  const uint32_t steps4 = (a.steps + 3) >> 2;
  const size_t lane_off = (size_t)(s >> 6) * steps4 * 256 + ((s & 63u) << 2);
  const uint32_t b_begin = a.step_begin >> 2;
  const uint32_t b_end = (a.step_end + 3) >> 2;
  const uint32_t dmax = a.dmax;

  // Prefetch: every block issues the same 2 + DCAP 16-byte loads per lane
  // (addresses clamped instead of branched around), so the compiler's
  // s_waitcnt for a block's data is a precise vmcnt(N) and never waits for
  // the next block's loads or for this block's scattered stores.
  const uint32_t* dotp = a.dot + lane_off;
  const uint32_t* hdrp = a.hdr + lane_off;
  const uint32_t* depp = (dmax ? a.deps : a.dot) + lane_off;
  const size_t plane = dmax ? a.plane : 0;
  const uint32_t jlast = dmax ? dmax - 1 : 0;
  const uint32_t b_last = b_end ? b_end - 1 : 0;
#define FX_LOAD(B, D, H, DP)                                                                 \
  do {                                                                                       \
    const size_t off_ = (size_t)min((B), b_last) * 256;                                      \
    D = *reinterpret_cast<const uint4*>(dotp + off_);                                        \
    H = *reinterpret_cast<const uint4*>(hdrp + off_);                                        \
    _Pragma("unroll") for (uint32_t j = 0; j < DCAP; ++j)                                    \
      DP[j] = *reinterpret_cast<const uint4*>(depp + (size_t)min(j, jlast) * plane + off_); \
  } while (0)

  uint4 cd, ch, nd_, nh;
  uint4 d0[DCAP], d1[DCAP];
  if (b_begin < b_end) FX_LOAD(b_begin, cd, ch, d0);

  for (uint32_t b = b_begin; b < b_end; ++b) {
    FX_LOAD(b + 1, nd_, nh, d1);
    const uint32_t base = b * 4;
    const uint32_t q0 = base < a.step_begin ? a.step_begin - base : 0u;
    const uint32_t q1 = a.step_end - base < 4u ? a.step_end - base : 4u;
    // Lanes progress through the block's steps independently: a lane starts
    // its next step as soon as its previous one (fast path or micro-op state
    // machine) is done, so the wavefront waits once per block for its slowest
    // lane instead of once per step.
    uint32_t q = q0;
    while (true) {
      const bool want = e.phase == PH_IDLE && q < q1 && !e.err && base + q < len;
      if (!__any(want || e.phase != PH_IDLE)) break;
      if (want) {
        const uint32_t m0 = lmask(q == 0), m1 = lmask(q == 1), m2 = lmask(q == 2), m3 = lmask(q == 3);
#define FX_PICK(V) (((V).x & m0) | ((V).y & m1) | ((V).z & m2) | ((V).w & m3))
        uint32_t rd[DCAP];
#pragma unroll
        for (uint32_t j = 0; j < DCAP; ++j) rd[j] = FX_PICK(d0[j]);
        e.step_start(base + q, FX_PICK(cd), FX_PICK(ch), rd, at_commit);
#undef FX_PICK
        ++q;
      }
      if (e.phase != PH_IDLE) e.slow_iter();
    }
    cd = nd_;
    ch = nh;
#pragma unroll
    for (uint32_t j = 0; j < DCAP; ++j) d0[j] = d1[j];
  }
#undef FX_LOAD

  if (!active) return;
  // Vertices still pending have no release step (yet).
  for (typename T::Mask m = e.occ; m; m &= m - 1) {
    const uint32_t sl = __builtin_ctzll((uint64_t)m);
    a.release[e.at(e.rec_of(sl) & 0x03FFFFFFu)] = FX_RELEASE_NONE;
  }
  a.nexec[s] = e.k;
  a.err[s] = e.err;
  if (a.flags & FX_FLAG_SAVE_STATE) {
    if constexpr (!T::GLOBAL) {
      for (uint32_t q = 0; q < T::MEM; ++q) gblock[q * WAVE + lane] = smem[q * WAVE + lane];
    }
    uint32_t* r = gblock + (size_t)T::MEM * WAVE + lane;
    r[0] = (uint32_t)(uint64_t)e.occ;
    r[WAVE] = (uint32_t)((uint64_t)e.occ >> 32);
    r[2 * WAVE] = (uint32_t)(uint64_t)e.wmask;
    r[3 * WAVE] = (uint32_t)((uint64_t)e.wmask >> 32);
    r[4 * WAVE] = e.k;
    r[5 * WAVE] = (e.err & 0xFFFFu) | (e.epoch << 16);
  }
}

// ------------------------------------------------------------ host side
// The tiers' face towards the tier table (SlotTier, fx_internal.h): which
// layout a tier number means is stated here, once.
template <uint32_t TIER> struct LayoutOf;
template <> struct LayoutOf<FX_TIER_LDS_LARGE> { using T = Tier1; };
template <> struct LayoutOf<FX_TIER_GLOBAL> { using T = Tier2; };
template <> struct LayoutOf<FX_TIER_LANE> { using T = TierLane; };

template <uint32_t TIER>
fx_tier_info SlotTier<TIER>::info(uint32_t) {
  using T = typename LayoutOf<TIER>::T;
  return {T::NSRC, T::P, 32 * T::XW, T::WORDS};
}

template <uint32_t TIER>
size_t SlotTier<TIER>::state_bytes(uint32_t, uint32_t lanes) {
  return (size_t)((lanes + WAVE - 1) / WAVE) * LayoutOf<TIER>::T::WORDS * WAVE * 4;
}

template <class T, uint32_t DCAP>
static int launch_exec_d(const KArgs& a, hipStream_t stream) {
  if (T::GLOBAL && !a.state) return FX_ERR_INVALID_ARG;
  const uint32_t blocks = (a.num_lanes + WAVE - 1) / WAVE;
  if (blocks == 0) return FX_OK;
  const size_t lds = T::GLOBAL ? 0 : (size_t)T::MEM * WAVE * 4;
  static bool configured = false;
  if (!configured && lds > 64 * 1024) {
    (void)hipFuncSetAttribute((const void*)k_graph_exec<T, DCAP>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    configured = true;
  }
  hipLaunchKernelGGL((k_graph_exec<T, DCAP>), dim3(blocks), dim3(WAVE), lds, stream, a);
  return hipGetLastError() == hipSuccess ? FX_OK : FX_ERR_HIP;
}

// deps of the incoming Add prefetched into registers: the smallest of 3/5/8
// that covers the batch's dep planes (more than 8 are read on demand)
template <uint32_t TIER>
int SlotTier<TIER>::launch(const KArgs& a, hipStream_t stream) {
  using T = typename LayoutOf<TIER>::T;
  if (a.dmax <= 3) return launch_exec_d<T, 3>(a, stream);
  if (a.dmax <= 5) return launch_exec_d<T, 5>(a, stream);
  return launch_exec_d<T, 8>(a, stream);
}

template <uint32_t TIER>
uint32_t SlotTier<TIER>::decode_pending(const uint32_t* block, uint32_t, uint32_t lane, uint32_t* dots,
                                        uint32_t* waits, uint32_t cap) {
  using T = typename LayoutOf<TIER>::T;
  const uint32_t* r = block + (size_t)T::MEM * WAVE + lane;
  const uint64_t occ = (uint64_t)r[0] | ((uint64_t)r[WAVE] << 32);
  const uint64_t wm = (uint64_t)r[2 * WAVE] | ((uint64_t)r[3 * WAVE] << 32);
  uint32_t c = 0;
  for (uint64_t m = occ; m; m &= m - 1) {
    const int sl = __builtin_ctzll(m);
    if (c < cap) {
      dots[c] = block[(T::DOT + sl) * WAVE + lane];
      waits[c] = ((wm >> sl) & 1) ? block[(T::WAIT + sl) * WAVE + lane] : 0u;
    }
    ++c;
  }
  return c;
}

template struct SlotTier<FX_TIER_LDS_LARGE>;
template struct SlotTier<FX_TIER_GLOBAL>;
template struct SlotTier<FX_TIER_LANE>;

}  // namespace fx
