/*
 * fantoch_amd.h — C-ABI drop-in boundary of the MI355X-native GraphExecutor.
 *
 * The reference has no FFI: its boundary is the Rust trait
 * `fantoch::executor::Executor` (fantoch/src/executor/mod.rs:27-89) implemented by
 * `GraphExecutor` (fantoch_ps/src/executor/graph/executor.rs:31-114) on top of
 * `DependencyGraph` (fantoch_ps/src/executor/graph/mod.rs:45-677).  Every entry
 * point below names the reference item it replaces.  Plain pointers and sizes
 * only; HIP streams are passed as `void*` (a `hipStream_t`); no torch types.
 *
 * Two surfaces:
 *   1. fx_graph_executor_*  — one executor handle, the `Executor` trait 1:1
 *      (handle -> to_clients -> metrics -> monitor).  Adds are buffered on the
 *      host and executed on the GPU when results are pulled.
 *   2. fx_batch_*           — thousands of independent commit streams (one per
 *      (instance, process) executor) executed by one kernel launch; the form
 *      the batched simulator and bench use.  Buffers are device pointers.
 *
 * Errors: the reference panics on invariant violations (mod.rs:220,234-237,258,
 * 263; tarjan.rs:245,255).  Here every entry point returns an `int` status
 * (FX_OK = 0); batched launches also fill a per-stream error word.
 */
#ifndef FANTOCH_AMD_H
#define FANTOCH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- status */
#define FX_OK 0
#define FX_ERR_INVALID_ARG 1   /* bad pointer/size/config                      */
#define FX_ERR_CAPACITY 2      /* per-stream pending table full, or (table
                                  executor) a vote range that leaves a gap
                                  beyond the tier's window above its voter's
                                  frontier: rerun the stream at a larger tier  */
#define FX_ERR_DOUBLE_INDEX 3  /* mod.rs:233-237 "tried to index already indexed" */
#define FX_ERR_DEPS_UNSORTED 4 /* deps plane not strictly ascending (canonical C1) */
#define FX_ERR_DOT_RANGE 5     /* source 0 / > n, or seq >= 2^24               */
#define FX_ERR_HIP 6           /* HIP runtime error (no device, launch failed) */
#define FX_ERR_UNSUPPORTED 7   /* shard_count > 1 request/reply path (out of scope) */
#define FX_ERR_ORDER_OVERFLOW 8/* more executions than order-plane rows        */
#define FX_ERR_TIME_RANGE 9    /* t_ms >= 2^24 relative to the stream base     */
#define FX_ERR_NO_DEVICE 10    /* no GPU visible: the product never falls back */
#define FX_ERR_LOG_FORMAT 11   /* malformed execution log (rw/mod.rs:90 `expect` panics) */
#define FX_ERR_SIM_CAPACITY 12 /* a simulated instance outgrew a table of its launch geometry
                                  (message ring, dot table, executor slots, clock window) */
#define FX_ERR_SIM_LATE 13     /* a simulated message found no state for its dot, or a
                                  reference assertion failed (runner.rs:239-241, single.rs:346-349) */
#define FX_ERR_SIM_EVENTS 14   /* a simulated instance exceeded its event budget */
#define FX_ERR_TIMEOUT 15      /* a drop-in handle's device wait passed its deadline
                                  (FX_HANDLE_TIMEOUT_MS, default 2000): the resident
                                  kernel was asked to stop; sticky for the handle */
#define FX_ERR_VOTE_RANGE 16   /* table executor: a vote range with a voter outside 1..n,
                                  start == 0, start > end (votes.rs:111), or no vote not
                                  seen before (table/mod.rs:180) */
#define FX_ERR_SLOT 17         /* slot executor: a slot that is 0, already executed
                                  (slot.rs:55) or already waiting (slot.rs:65-66) */

/* ------------------------------------------------- packed stream format */
/* A dot (fantoch/src/id.rs:21-27, Id<u8>{source, sequence}, derived Ord) is
 * packed as (source << 24) | seq; the packed u32 orders exactly like the
 * reference's (source, sequence) tuple. */
#define FX_SEQ_BITS 24u
#define FX_SEQ_MASK 0x00FFFFFFu
#define FX_PACK_DOT(src, seq) ((((uint32_t)(src)) << FX_SEQ_BITS) | ((uint32_t)(seq) & FX_SEQ_MASK))
#define FX_DOT_SRC(d) ((uint32_t)(d) >> FX_SEQ_BITS)
#define FX_DOT_SEQ(d) ((uint32_t)(d) & FX_SEQ_MASK)

/* Record header word: t_ms (24 bits) | ndeps (5 bits) | kind (3 bits). */
#define FX_HDR_T(h) ((uint32_t)(h) & 0x00FFFFFFu)
#define FX_HDR_ND(h) (((uint32_t)(h) >> 24) & 31u)
#define FX_HDR_KIND(h) ((uint32_t)(h) >> 29)
#define FX_MAKE_HDR(t, nd, kind) \
  (((uint32_t)(t) & 0x00FFFFFFu) | (((uint32_t)(nd) & 31u) << 24) | (((uint32_t)(kind) & 7u) << 29))
#define FX_KIND_ADD 0u        /* GraphExecutionInfo::Add -> handle_add (mod.rs:213-275) */
#define FX_KIND_INDEX_ONLY 1u /* VertexIndex::index without a search (index.rs:33-37);
                                 the hook the reference's sccs_found_and_missing_dep test uses */
#define FX_KIND_EXECUTED 2u   /* RequestReply::Executed{dot} (mod.rs:394-402): executed-clock
                                 add + check_pending; partial replication only */

/* Order-plane word: arrival index of the executed command | SCC-start flag. */
#define FX_ORDER_SCC_START 0x80000000u
#define FX_ORDER_REC(o) ((uint32_t)(o) & 0x7FFFFFFFu)
#define FX_RELEASE_NONE 0xFFFFFFFFu

/* Batch flags */
#define FX_FLAG_INIT 1u              /* start from an empty executor (else resume from state) */
#define FX_FLAG_EXECUTE_AT_COMMIT 2u /* Config::execute_at_commit (executor.rs:72-73)    */
#define FX_FLAG_SAVE_STATE 4u        /* write the executor state back for a later resume */
#define FX_FLAG_PARTIAL 8u           /* partial replication (shard_count > 1): the first search
                                        of an Add collects every missing dep (tarjan.rs:148-166),
                                        a vertex waits on all of them; FX_TIER_WIDE_HBM only,
                                        through fx_batch_execute_partial */
/* fx_batch_run_tiered only: first tier = ((flags >> FX_FLAG_TIER_SHIFT) & 15) - 1
 * (0 = the default tier, FX_TIER_DEFAULT). */
#define FX_FLAG_TIER_SHIFT 8u
#define FX_FLAG_FIRST_TIER(t) ((((uint32_t)(t)) + 1u) << FX_FLAG_TIER_SHIFT)

/* Plane layout.  Every per-(step, stream) array ("plane") is tiled in tiles
 * of 64 streams x 4 steps (1 KiB): element (step, stream) lives at
 *   fx_index(step, stream, steps) =
 *     ((stream / 64) * ceil(steps / 4) + step / 4) * 256 + (stream % 64) * 4 + step % 4
 * so one 16-byte load per lane fetches 4 consecutive steps of that lane's
 * stream and the 64 lanes of a wavefront (= 64 streams) read 1 KiB contiguous
 * per plane per 4 steps.  A plane holds fx_plane_words(S, steps) u32 words
 * (S rounded up to 64, steps to 4).  dep j of (step, stream) lives at
 * deps[j * fx_plane_words(S, steps) + fx_index(step, stream, steps)]; the
 * deps of one record are strictly ascending by packed dot (canonical C1,
 * replacing the hash order of executor.rs:76). */
#define FX_TILE_STREAMS 64u
#define FX_TILE_STEPS 4u
#if defined(__HIPCC__)
#define FX_INLINE __host__ __device__ static inline
#else
#define FX_INLINE static inline
#endif
FX_INLINE size_t fx_plane_words(uint32_t num_streams, uint32_t steps) {
  return (size_t)((num_streams + 63u) / 64u) * 64u * (size_t)((steps + 3u) / 4u) * 4u;
}
FX_INLINE size_t fx_index(uint32_t step, uint32_t stream, uint32_t steps) {
  return ((size_t)(stream >> 6) * ((steps + 3u) >> 2) + (step >> 2)) * 256u +
         ((stream & 63u) << 2) + (step & 3u);
}
typedef struct fx_stream_batch {
  const uint32_t* dot;      /* plane: packed dot of the Add                */
  const uint32_t* hdr;      /* plane: FX_MAKE_HDR(t_ms, ndeps, kind)       */
  const uint32_t* deps;     /* dmax planes: packed dep dots, ascending     */
  const uint32_t* lengths;  /* [S] valid steps per stream, or NULL = steps */
  uint32_t num_streams;     /* S                                           */
  uint32_t steps;           /* rows per plane                              */
  uint32_t dmax;            /* number of dep planes                        */
  uint32_t n;               /* processes per instance (sources 1..n)       */
} fx_stream_batch;

typedef struct fx_order_batch {
  uint32_t* order;    /* plane, row k: k-th executed command: arrival index | SCC_START */
  uint32_t* release;  /* plane, row a: step at which arrival a was executed, or NONE;
                         rows of arrivals a stream did not process (err != 0, or
                         beyond its length) are left untouched                 */
  uint32_t* nexec;    /* [S] number of executed commands                            */
  uint32_t* err;      /* [S] FX_* status of the stream                              */
} fx_order_batch;

/* Dense histograms (fantoch/src/metrics/histogram.rs:14-59 keeps an exact
 * BTreeMap; values here are small integers so a dense array is exact as long
 * as every value < nbins; the last bin counts values >= nbins-1). */
typedef struct fx_hist_batch {
  uint64_t* chain_size;       /* ExecutorMetricsKind::ChainSize (mod.rs:492-493)      */
  uint32_t nbins_chain;
  uint64_t* execution_delay;  /* ExecutorMetricsKind::ExecutionDelay (mod.rs:514-518) */
  uint32_t nbins_delay;
} fx_hist_batch;

/* Executor tiers: capacity of the per-stream pending table and of the
 * executed-clock window above each source's frontier.  A stream that exceeds
 * its tier stops with FX_ERR_CAPACITY and is rerun at the next tier
 * (fx_batch_run_tiered escalates 0 -> 1 -> 2, 3 -> 1 -> 2, 4 -> 2, 5 -> 1 -> 2,
 * 6 -> 1 -> 2, and then 2 -> 7 -> 8). */
#define FX_TIER_GROUP 0      /* 16 lanes per stream: 16 pending, 8 cached deps, n <= 16 */
#define FX_TIER_LDS_LARGE 1  /* lane per stream, LDS-resident: 32 pending, one wave per CU */
#define FX_TIER_GLOBAL 2     /* lane per stream, HBM-resident: 64 pending, 1024-bit windows */
#define FX_TIER_LANE 3       /* lane per stream, LDS-resident: 12 pending (alternative tier 0) */
#define FX_TIER_WAVE 4       /* one wavefront per stream: 64 pending, 8 cached deps, <= 14 deps */
#define FX_TIER_LANE_REG 5   /* lane per stream, register-resident slot table, lanes progress
                                independently: 12 pending, n <= 8, <= 8 deps */
#define FX_TIER_SPLIT 6      /* per 64-stream tile: tier 5 for tiles with few deps per Add,
                                tier 0 for dense ones, both launched concurrently; whole
                                batches only (FX_FLAG_INIT, no stream_map, no saved state);
                                `state` = fx_batch_state_bytes(6, n, S) bytes of scratch */
#define FX_TIER_WIDE 7       /* one wavefront per stream, the graph as tables in LDS: 512
                                pending, 1024-bit windows (rerun tier after tier 2) */
#define FX_TIER_WIDE_HBM 8   /* the same over HBM tables: 16384 pending, 32768-bit windows;
                                `state` = fx_batch_state_bytes(8, n, lanes) bytes; the one
                                wide tier that resumes (FX_FLAG_SAVE_STATE / no FX_FLAG_INIT) */
#define FX_NUM_TIERS 9
#define FX_TIER_DEFAULT FX_TIER_SPLIT

typedef struct fx_tier_info {
  uint32_t max_sources;    /* n supported                                   */
  uint32_t pending_cap;    /* vertices pending at once                       */
  uint32_t window_bits;    /* executed-clock exceptions above the frontier  */
  uint32_t state_words;    /* 32-bit state words per stream                  */
} fx_tier_info;

/* ---------------------------------------------------- batched executor */

/* Capacity of a tier for n processes. Replaces nothing in the reference (its
 * HashMap/DashMap indexes are unbounded, index.rs:18-51,145-208). */
int fx_tier_query(uint32_t tier, uint32_t n, fx_tier_info* out);

/* Bytes of resumable executor state for num_streams streams at a tier. */
size_t fx_batch_state_bytes(uint32_t tier, uint32_t n, uint32_t num_streams);

/* Run GraphExecutor::handle(Add) (executor.rs:69-93) for steps
 * [step_begin, step_end) of every stream, i.e. DependencyGraph::handle_add
 * (mod.rs:213-275) -> find_scc (409-486) -> TarjanSCCFinder::strong_connect
 * (tarjan.rs:96-316) -> save_scc (488-523) -> index_pending/check_pending/
 * try_pending (525-642), with canonical iteration C1 (deps ascending) and C2
 * (waiters ascending).
 *   stream_map: NULL, or [num_lanes] stream indices to run (tier reruns)
 *   state:      device buffer of fx_batch_state_bytes(tier, n, num_lanes)
 *               (NULL allowed with FX_FLAG_INIT and without FX_FLAG_SAVE_STATE)
 *   init_frontier: NULL, or [num_streams][8] executed-clock frontiers to start
 *               from (AboveExSet::from_events(1..=f), mod.rs:1309-1315),
 *               indexed by stream (not lane)
 * All pointers are device pointers; the call is asynchronous on hip_stream. */
int fx_batch_execute(const fx_stream_batch* in, const fx_order_batch* out,
                     uint32_t tier, const uint32_t* stream_map, uint32_t num_lanes,
                     void* state, uint32_t step_begin, uint32_t step_end,
                     uint32_t flags, const uint32_t* init_frontier, void* hip_stream);

/* Fold the executor metrics of a finished batch into dense histograms
 * (Metrics::collect, fantoch/src/metrics/mod.rs:34-48): one ChainSize sample
 * per SCC and one ExecutionDelay = t(release) - t(add) sample per executed
 * command.  Histogram buffers are accumulated into (zero them first): a call
 * adds its samples to what the bins hold and writes no word beyond them.
 *
 * Row by row: for stream s, ne = nexec[s]; for each order row k < ne, with
 *   rec = FX_ORDER_REC(order[k]) and rs = release[rec] (read only if rec < steps),
 * - the row gives one ExecutionDelay sample iff rec < steps and rs < steps (so
 *   FX_RELEASE_NONE gives none): (FX_HDR_T(hdr[rs]) - FX_HDR_T(hdr[rec])) as a
 *   uint32_t (a release before the arrival wraps), counted in bin
 *   min(sample, nbins_delay - 1);
 * - a row that gives a delay sample and carries FX_ORDER_SCC_START also gives
 *   one ChainSize sample: 1 + the rows without the flag that follow it below
 *   ne (whether or not those give a delay sample), counted in bin
 *   min(size, nbins_chain - 1).  Rows before a stream's first flagged row, and
 *   the rows behind a flagged row that gives no delay sample, belong to no SCC.
 * Order rows at or above ne, release rows no counted row names, the header
 * bits 24..31 and the pad rows and streams of the planes have no influence;
 * lengths, dot, deps, dmax, n and out->err are not read and may be null / 0.
 * Guards: a stream with nexec[s] > steps contributes no sample (nothing a
 * driver wrote: no row index leaves the plane, the stream has no status to
 * report it in); a null batch, output or histogram struct, a null in->hdr,
 * out->order, out->release, out->nexec or histogram buffer, or nbins < 2 on
 * either histogram is refused with FX_ERR_INVALID_ARG before the device is
 * looked for.  No stream or no step: FX_OK, nothing read or written.
 * Asynchronous on hip_stream; device pointers. */
int fx_batch_metrics(const fx_stream_batch* in, const fx_order_batch* out,
                     const fx_hist_batch* hists, void* hip_stream);
/* The same over host memory (the host twin: same checks, same samples, same
 * guards); synchronous. */
int fx_batch_metrics_host(const fx_stream_batch* in, const fx_order_batch* out,
                          const fx_hist_batch* hists);

/* Synchronous convenience driver: runs every stream at the first tier
 * (FX_TIER_DEFAULT unless FX_FLAG_FIRST_TIER(t) is set) and reruns the streams
 * that report FX_ERR_CAPACITY up the escalation chain.  Device pointers.
 * Returns FX_OK when every stream finished with FX_OK. */
int fx_batch_run_tiered(const fx_stream_batch* in, const fx_order_batch* out,
                        uint32_t flags, void* hip_stream, uint32_t* tier_counts);

/* Quiescent-cut driver for huge streams (BASELINE configs[4]): every stream is
 * split after each step t whose prefix is dependency-closed (every dep of an
 * Add at a step <= t was added at a step <= t); there the reference's
 * DependencyGraph (graph/mod.rs:213-642) has executed the whole prefix and
 * holds nothing pending, so each segment runs from an empty graph with its
 * prefix deps dropped and its dots renumbered per source (order-preserving).
 * Segments longer than one Add run as one batch through fx_batch_run_tiered
 * and map back; a one-Add segment executes at its own step.
 * A stream without a usable decomposition (a dep that never arrives, a
 * segment over 4096 steps, a double index, an index-only record) or whose
 * segments do not all execute completely runs whole through
 * fx_batch_run_tiered.  Output planes are identical to fx_batch_run_tiered's.
 * Synchronous; device pointers. */
typedef struct fx_cut_stats {
  uint64_t segments;                    /* segments executed as independent streams:
                                           those of the streams that were cut (a
                                           stream that runs whole counts in neither
                                           segments, single_segments nor max_segment) */
  uint32_t max_segment;                 /* longest segment (steps) of a cut stream   */
  uint32_t whole_streams;               /* streams run whole (all reasons)          */
  uint32_t failed_streams;              /* ... of which because a segment did not
                                           execute completely (capacity, or the cut
                                           argument failing: never seen so far)     */
  uint32_t tier_counts[16];             /* segment-batch streams run per tier       */
  uint64_t single_segments;             /* of `segments`, those one Add long: executed
                                           at their own step without the batch (a
                                           singleton SCC after the executed prefix);
                                           single_segments <= segments             */
} fx_cut_stats;
int fx_batch_run_cut(const fx_stream_batch* in, const fx_order_batch* out, uint32_t flags, void* hip_stream,
                     fx_cut_stats* stats);

/* ---------------------------------------- predecessors executor (Caesar) */
/* PredecessorsExecutor (fantoch_ps/src/executor/pred/{mod,index,executor}.rs):
 * commit streams as fx_stream_batch plus each Add's Caesar clock
 * (common/pred/clocks/mod.rs:15-30: (seq, process id), lexicographic) packed
 * as (seq << 8) | id in two planes (low / high 32 bits).  Phase one waits for
 * every dep to commit, phase two for every dep with a lower clock to execute;
 * the waiters of a removed PendingIndex entry are visited ascending by dot.
 * Outputs as the batched GraphExecutor: order row k = arrival index of the
 * k-th executed command (| FX_ORDER_SCC_START: every command its own group),
 * release[arrival] = executing step; fx_batch_metrics gives ExecutionDelay. */
#define FX_PRED_MAX_DEPS 256u
typedef struct fx_pred_batch {
  fx_stream_batch base;       /* dot / hdr / deps / lengths planes, S, steps, dmax, n */
  const uint32_t* clock_lo;   /* plane: low 32 bits of (clock seq << 8 | process id) */
  const uint32_t* clock_hi;   /* plane: high 32 bits                                */
  const uint32_t* ndeps;      /* plane: deps per Add (Caesar commits carry every
                                 conflicting command: up to FX_PRED_MAX_DEPS), or
                                 NULL = FX_HDR_ND (dmax <= 31) */
} fx_pred_batch;
/* Table tiers: SMALL = LDS, 64 pending (many wavefronts per CU; at n = 5 and
 * dmax = 5 also 32 dot-index slots per source, 256-seq clock windows and a
 * 32-deep recursion, so such streams reach FX_ERR_CAPACITY sooner); LDS = LDS,
 * the most of 512 / 256 / 128 pending that fit (FX_ERR_UNSUPPORTED if none
 * does); HBM = tables in `state` (fx_pred_state_bytes), 8192 pending.
 * A stream that outgrows a table stops at that row with FX_ERR_CAPACITY:
 * what executed before the failing operation stands (order, release, nexec),
 * the operation itself records nothing -- a commit beyond the committed
 * window executes nothing, FX_FLAG_EXECUTE_AT_COMMIT included, and neither
 * does an execution beyond the executed window.  The recursion depth is
 * tested before a PendingIndex::remove looks for its waiters, so at the
 * depth limit a removal that would find none stops the stream as well
 * (unless that phase's index is empty); fx_pred_run reruns such a stream. */
#define FX_PRED_TIER_SMALL 0u
#define FX_PRED_TIER_LDS 1u
#define FX_PRED_TIER_HBM 2u
/* One launch over num_lanes streams (stream_map NULL = all) at one table
 * tier.  Streams that run out report FX_ERR_CAPACITY.  Whole streams, from an
 * empty executor; flags: FX_FLAG_EXECUTE_AT_COMMIT. */
int fx_pred_execute(const fx_pred_batch* in, const fx_order_batch* out, const uint32_t* stream_map,
                    uint32_t num_lanes, uint32_t tier, void* state, uint32_t flags, void* hip_stream);
size_t fx_pred_state_bytes(uint32_t n, uint32_t dmax, uint32_t lanes);
/* Synchronous driver: every stream at SMALL, then the streams that ran out of
 * capacity at LDS, then HBM; *reruns (optional) = stream reruns in total. */
int fx_pred_run(const fx_pred_batch* in, const fx_order_batch* out, uint32_t flags, void* hip_stream,
                uint32_t* reruns);
/* Resumable streams: the predecessors executor fed in pieces (the reference's
 * executor handles one PredecessorsExecutionInfo at a time, pred/executor.rs).
 * fx_pred_advance runs rows [done, len) of every stream -- len = lengths[s]
 * capped at steps, or steps (lengths NULL); done = where the stream's previous
 * call stopped (0 with FX_FLAG_INIT, which starts the stream from an empty
 * executor whatever `state` holds; the call clears the tables itself).  The
 * planes are the whole stream's planes and arrival indices are plane rows.
 * Rows outside [done, len) influence nothing (the kernel may load the 4-row
 * tile that holds done and the tile after len, which lie inside the padded
 * plane).
 * tier: FX_PRED_TIER_SMALL, _LDS or _HBM; the session uses exactly the tables
 * fx_pred_execute uses at that tier for that n and dmax (SMALL at n = 5,
 * dmax = 5: the compiled layout and its limits).  A tier whose tables do not
 * fit: fx_pred_session_bytes == 0 and FX_ERR_UNSUPPORTED.
 * The outputs are fx_pred_execute's and are cumulative: order row k is the
 * k-th executed command since row 0, nexec the running total.  After every
 * call, for any partition into calls, every word of order, release, nexec and
 * err equals what one fx_pred_execute at the same tier with this call's
 * lengths leaves on buffers of the same initial content, the words such a call
 * does not write included (release of rows not yet executed, order rows from
 * nexec on, rows past len, pad rows and pad streams).
 *   len == done  nothing but the stream's state header is read; nexec[s] and
 *                err[s] are rewritten with their current values
 *   len < done   err[s] = FX_ERR_INVALID_ARG, nexec[s] keeps its value, state
 *                as it was: a later call with len >= done continues
 * steps, n, dmax, tier, the presence of the ndeps plane and
 * FX_FLAG_EXECUTE_AT_COMMIT are fixed for a session: they live in the stream's
 * state header beside a tag, and the header is validated before a table is
 * touched.  A wrong tag (a state that never saw FX_FLAG_INIT), a differing
 * fixed value, done > steps, nexec > done or nfree above the tier's vertices:
 * err[s] = FX_ERR_INVALID_ARG, state as it was, nothing else of the stream
 * written.  A stream that stopped with any error stays stopped: later calls
 * handle nothing for it and report the same err and nexec.  FX_ERR_CAPACITY is
 * final for the session (no promotion to a larger tier).
 * Refused with FX_ERR_INVALID_ARG before any launch or store: a null in, out
 * or state, a null plane pointer, every argument fx_pred_execute refuses (n,
 * dmax, steps, ndeps versus dmax > 31), tier > FX_PRED_TIER_HBM, flags other
 * than FX_FLAG_INIT | FX_FLAG_EXECUTE_AT_COMMIT.  After those checks no device
 * gives FX_ERR_NO_DEVICE (the device entry only); num_streams == 0 or steps ==
 * 0 returns FX_OK and does nothing.
 * state: fx_pred_session_bytes(tier, n, dmax, num_streams) bytes, 16-byte
 * aligned, indexed by stream (no stream_map): num_streams headers, then per
 * stream one contiguous image of the tables (about 1,150 words at the compiled
 * SMALL layout; at HBM the tables are used in place and the image also holds
 * their scratch).  It belongs to the side (device or host) that initialised
 * it.  Asynchronous on hip_stream; profile slot FX_PROFILE_SLOT_PRED + 3. */
size_t fx_pred_session_bytes(uint32_t tier, uint32_t n, uint32_t dmax, uint32_t num_streams);
int fx_pred_advance(const fx_pred_batch* in, const fx_order_batch* out, uint32_t tier, void* state, uint32_t flags,
                    void* hip_stream);
/* The same on the host (host pointers, a state of its own): the same output
 * bytes for the same sequence of calls.  No device needed. */
int fx_pred_advance_host(const fx_pred_batch* in, const fx_order_batch* out, uint32_t tier, void* state,
                         uint32_t flags);

/* ------------------------------------------------ table executor (Tempo) */
/* TableExecutor (fantoch_ps/src/executor/table/{mod,executor}.rs) with
 * shard_count = 1 and single-key commands: a stream is the sequence of
 * TableExecutionInfo values one executor handles.  Keys are dense ids
 * 0..keys-1 (interning is the caller's job); each key owns a VotesTable
 * (mod.rs:104-267): per process 1..n the votes seen (a frontier = the highest
 * c with every vote 1..c seen, plus the votes above it; the ARClock of
 * mod.rs:112,127-128) and the pending ops sorted by (clock, dot).
 *   attached  AttachedVotes{dot, clock, key, votes} (mod.rs:141-169): the op
 *             is inserted under (clock, dot), whose slot must be free
 *             (FX_ERR_DOUBLE_INDEX while the earlier one is pending), then
 *             the votes are added
 *   detached  DetachedVotes{key, votes} (mod.rs:171-194): votes only
 * Every vote range must add a vote not seen before (mod.rs:180), have
 * 1 <= start <= end (votes.rs:111) and a voter in 1..n: FX_ERR_VOTE_RANGE.
 * After either event, on that key (mod.rs:196-266): stable clock = element
 * n - stability_threshold of the n frontiers sorted ascending; every pending
 * op of the key with clock <= stable clock executes, ascending by
 * (clock, dot).  (split_off's bound (stable + 1, Dot(1, 1)) is excluded and
 * no dot sorts below (1, 1), so `clock <= stable` is exact.)
 * FX_FLAG_EXECUTE_AT_COMMIT (executor.rs:125-139): an attached command
 * executes at its own step and every vote is ignored.
 * Multi-key commands and the StableAtShard messages an executor sends itself
 * (executor.rs:168-359) are the _mk entry points below; commands that span
 * shards (shard_count > 1: StableAtShard from and to other executors) are the
 * _ps entry points below those.
 * Streams fed in pieces (from which a host routes StableAtShard between the
 * executors of a group as it goes): fx_table_advance, below those; the same
 * closed loop inside one kernel launch: fx_table_run_groups, last.
 * Out of scope: a Tempo simulator, a single-executor handle, and clocks or
 * votes at or above 2^32 (Tempo's clocks count commands).
 *
 * Header word: key (24 bits) | votes in the event (7 bits) | kind (1 bit). */
#define FX_TABLE_ATTACHED 0u
#define FX_TABLE_DETACHED 1u
#define FX_TABLE_MAX_VOTES 64u
#define FX_TABLE_MAX_KEYS (1u << 24)
#define FX_TABLE_HDR(kind, nvotes, key) \
  ((((uint32_t)(kind) & 1u) << 31) | (((uint32_t)(nvotes) & 127u) << 24) | ((uint32_t)(key) & 0x00FFFFFFu))
#define FX_TABLE_HDR_KIND(h) ((uint32_t)(h) >> 31)
#define FX_TABLE_HDR_NVOTES(h) (((uint32_t)(h) >> 24) & 127u)
#define FX_TABLE_HDR_KEY(h) ((uint32_t)(h) & 0x00FFFFFFu)
typedef struct fx_table_batch {
  const uint32_t* hdr;      /* plane: FX_TABLE_HDR(kind, nvotes, key)                   */
  const uint32_t* dot;      /* plane: packed dot (attached events only)                 */
  const uint32_t* clock;    /* plane: commit clock (attached events only)               */
  const uint32_t* votes;    /* 3 * vmax planes: slot j = planes 3j (voter), 3j + 1
                               (start), 3j + 2 (end); plane p of (step, stream) at
                               votes[p * fx_plane_words(S, steps) + fx_index(...)]      */
  const uint32_t* lengths;  /* [S] valid steps per stream, or NULL = steps              */
  uint32_t num_streams;     /* S                                                        */
  uint32_t steps;           /* rows per plane                                           */
  uint32_t n;               /* processes (voters 1..n), 1..16                           */
  uint32_t keys;            /* dense key ids 0..keys-1, 1..FX_TABLE_MAX_KEYS            */
  uint32_t vmax;            /* vote slots per event, 1..FX_TABLE_MAX_VOTES              */
  uint32_t stability_threshold; /* 1..n (fx_tempo_quorum_sizes)                         */
} fx_table_batch;
/* Tiers.  Capacities per stream:
 *   ONCHIP  votes tables in LDS, pending ops in registers: 64 pending ops,
 *           keys <= 32 (FX_ERR_UNSUPPORTED for more), a vote may lie at most
 *           32 above its voter's frontier on that key
 *   HBM     votes tables in `state` (fx_table_state_bytes): 512 pending ops,
 *           any key count; a vote range that leaves a gap above its voter's
 *           frontier may end at most 2048 above it.  A range that starts at
 *           or below the frontier + 1 may be of any length: it holds nothing
 *           above the frontier, it only moves it (Tempo bumps a rarely used
 *           key to the highest clock of a command, so such ranges are long)
 * The windows limit the gaps, not the clocks: clocks and votes run to
 * 2^32 - 1 on both tiers.  A stream that outgrows a tier stops with
 * FX_ERR_CAPACITY and reruns whole at the next (on the ONCHIP tier of
 * fx_table_execute that includes a range from the frontier that ends more
 * than 32 above it); HBM is the last tier, there the status stays.  A stream
 * never produces a wrong order. */
#define FX_TABLE_TIER_ONCHIP 0u
#define FX_TABLE_TIER_HBM 1u
#define FX_TABLE_ONCHIP_PENDING 64u
#define FX_TABLE_ONCHIP_KEYS 32u
#define FX_TABLE_ONCHIP_WINDOW 32u
#define FX_TABLE_HBM_PENDING 512u
#define FX_TABLE_HBM_WINDOW 2048u
/* One launch over num_lanes streams (stream_map NULL = all) at one tier.
 * Outputs as fx_pred_execute: order row k = arrival index of the k-th
 * executed command | FX_ORDER_SCC_START, release[a] = the step that executed
 * arrival a (rows of detached events and of never-executed commands are not
 * written: fill with FX_RELEASE_NONE), nexec and err per stream.  A failing
 * stream stops at that event; its rows for earlier events stay valid.
 * stable_clock: NULL, or [S * keys]: each key's stable clock after the
 * stream's last processed event (0 for a key never seen).  Whole streams from
 * an empty executor; flags: FX_FLAG_EXECUTE_AT_COMMIT.  Asynchronous. */
int fx_table_execute(const fx_table_batch* in, const fx_order_batch* out, uint32_t* stable_clock,
                     const uint32_t* stream_map, uint32_t num_lanes, uint32_t tier, void* state, uint32_t flags,
                     void* hip_stream);
size_t fx_table_state_bytes(uint32_t n, uint32_t keys, uint32_t lanes);
/* Synchronous driver: every stream at ONCHIP (skipped when keys do not fit),
 * then the streams that ran out of capacity at HBM; *reruns (optional) =
 * stream reruns in total. */
int fx_table_run(const fx_table_batch* in, const fx_order_batch* out, uint32_t* stable_clock, uint32_t flags,
                 void* hip_stream, uint32_t* reruns);

/* Multi-key commands (shard_count = 1: every key of a command is on this
 * shard).  Tempo emits one AttachedVotes per key of a command
 * (fantoch_ps/src/protocol/tempo.rs:614-636), so a command with K keys is K
 * attached events with the same dot and clock, each with its key and that
 * key's votes; the plane `nkeys` holds K for every attached event
 * (1..FX_TABLE_MAX_CMD_KEYS, else FX_ERR_INVALID_ARG; ignored for detached
 * events).  The command's rifl is its dot.
 *
 * Per key a FIFO of the ops that left the votes table and have not executed
 * (PendingPerKey, executor.rs:33-37).  After an event on key k the ops the
 * votes table releases, ascending by (clock, dot): if k's queue is not empty
 * they join it; otherwise they are tried in order and the first that cannot
 * execute is queued with the rest behind it, untried (executor.rs:237-277).
 * Trying an op (executor.rs:280-359): a single-key op executes; an op of a
 * K-key command adds one to the command's stable count, and when that reaches
 * K, one StableAtShard(other key, rifl) per other key of the command goes onto
 * to_executors -- in ascending key id, a rule of this library (DESIGN.md 1.1,
 * C13), the reference iterates a HashMap -- the count is dropped and the op
 * executes; before that it waits at the head of its queue.
 * StableAtShard(key, rifl) (executor.rs:168-235): if the head of key's queue
 * is rifl it executes and the ops behind it are tried until one cannot
 * execute; otherwise the message is buffered for that (key, rifl) and counted
 * when the op is tried (executor.rs:345-347).
 * After every event (fantoch/src/sim/runner.rs:405-419) to_executors is popped
 * until empty, last pushed first, and each popped message is handled once;
 * messages pushed meanwhile wait for the next event, and messages left after
 * the stream's last event are never handled (their ops stay unexecuted).
 *
 * Outputs as fx_table_execute with one order row and one release row per
 * executed (command, key) partial, as the reference has one ExecutorResult
 * per (rifl, key): order row k = the event row of the k-th executed partial |
 * FX_ORDER_SCC_START; release[a] = the event during whose handling or drain
 * the partial of event a executed; nexec counts partials.
 * FX_FLAG_EXECUTE_AT_COMMIT executes every attached event at its own step.
 *
 * Within a stream the events of one dot must carry the same K and clock, use
 * distinct keys and number at most K.  Checked when an attached event arrives,
 * against the events of its dot whose partials have not executed yet
 * (FX_ERR_INVALID_ARG, the stream stops): another K, another clock, the same
 * key (FX_ERR_DOUBLE_INDEX while that op is still in the votes table), K such
 * events already, or one of them already told that the command is stable at
 * the shard (K events came before).  Not caught: an event of a dot whose
 * earlier partials have all executed -- it starts a command of its own.
 *
 * Capacities per stream: votes tables as fx_table_execute, except that on the
 * ONCHIP tier a vote range that starts at or below its voter's frontier + 1
 * may be of any length (it only moves the frontier; Tempo bumps a key's clock
 * to the highest of a command's keys, so such ranges are long); the ops that have
 * arrived and not executed (votes tables plus queues) FX_TABLE_MK_*_LIVE;
 * to_executors FX_TABLE_MK_*_STACK entries (every message on it belongs to a
 * live op, so the live limit is reached first); buffered (key, rifl) pairs
 * FX_TABLE_MK_BUFFERED.  Beyond a limit the stream stops with FX_ERR_CAPACITY
 * and fx_table_run_mk reruns it whole on the HBM tier. */
#define FX_TABLE_MAX_CMD_KEYS 8u
#define FX_TABLE_MK_ONCHIP_LIVE 64u
#define FX_TABLE_MK_HBM_LIVE 512u
#define FX_TABLE_MK_ONCHIP_STACK 64u
#define FX_TABLE_MK_HBM_STACK 512u
#define FX_TABLE_MK_BUFFERED 64u
typedef struct fx_table_batch_mk {
  fx_table_batch base;
  const uint32_t* nkeys;    /* plane: keys of the event's command (attached events)     */
} fx_table_batch_mk;
/* As fx_table_execute / fx_table_run (same state size, same profile slots). */
int fx_table_execute_mk(const fx_table_batch_mk* in, const fx_order_batch* out, uint32_t* stable_clock,
                        const uint32_t* stream_map, uint32_t num_lanes, uint32_t tier, void* state, uint32_t flags,
                        void* hip_stream);
int fx_table_run_mk(const fx_table_batch_mk* in, const fx_order_batch* out, uint32_t* stable_clock, uint32_t flags,
                    void* hip_stream, uint32_t* reruns);

/* Commands that span shards (shard_count > 1).  A stream is still what one
 * executor handles, in order; that now includes the StableAtShard messages
 * other shards' executors sent it, and one more output says when a command
 * became stable at this shard, from which the host makes the messages it
 * routes to the other shards.  Messages to the executor's own shard keep the
 * _mk drain unchanged.
 *
 * Inputs: fx_table_batch_mk, where the `nkeys` word of an attached event is
 * FX_TABLE_PS_WORD(nkeys, shards): nkeys = the command's keys at this shard
 * (shard_key_count, executor.rs:57-60), 1..FX_TABLE_MAX_CMD_KEYS; shards = the
 * shards the command accesses, this one included (shard_to_keys.len(), :61),
 * 1..FX_TABLE_MAX_CMD_SHARDS; anything else is FX_ERR_INVALID_ARG.  A third
 * event, FX_TABLE_HDR_STABLE(key) -- kind FX_TABLE_DETACHED with the vote-count
 * field at 127, which the other entry points refuse -- is a
 * StableAtShard{key, rifl} from another shard (:140-142): the rifl (the
 * command's dot, FX_ERR_DOT_RANGE outside 1..n / seq 0) is in the `dot` plane;
 * the clock plane, the vote planes and nkeys are ignored.
 *
 * Semantics, beside those of _mk:
 *   attached  missing_stable_shards = shards (:61); the op is single-key only
 *             if shards == 1 && nkeys == 1 (:71-75, :290-293)
 *   trying an op with nkeys == 1 and shards > 1 (:311-316): the command is
 *             stable here at once, missing_stable_shards -= 1
 *   trying an op with nkeys > 1 (:319-341): the stable count as in _mk; the
 *             partial whose try makes it nkeys is the sender: the other keys
 *             at this shard are told through to_executors in ascending key id
 *             (C13), missing_stable_shards -= 1.  The keys at other shards are
 *             the host's to route
 *   then      a buffered count for (key, rifl) is removed and subtracted
 *             (:345-347).  A count above missing_stable_shards -- the
 *             reference's usize would underflow -- stops the stream with
 *             FX_ERR_INVALID_ARG before anything of that try is written (what
 *             the same event executed before it stays)
 *   then      the op executes at missing_stable_shards == 0 (:349-352) and is
 *             otherwise handed back as its queue's head (:353-357)
 *   StableAtShard event: handled exactly as a popped message (:168-235).  If
 *             it names the head of the key's queue, missing_stable_shards -= 1
 *             (:177), and at 0 the head executes and the queue runs on
 *             (:186-217); otherwise -- the queue is empty, the op is still in
 *             the votes table, it is queued behind another head, or it never
 *             arrives -- the count buffered for (key, rifl) goes up by one
 *             (:219-233).  The usual drain follows.  Under
 *             FX_FLAG_EXECUTE_AT_COMMIT the event has no effect (:125-126)
 * Not caught: a message beyond the shards - 1 that other shards can send, for
 * a head whose own shard is not stable yet, takes its count to 0 and executes
 * it early, as the reference would; what the command's other partials at this
 * shard then do is not specified.
 *
 * Outputs: order, release, nexec, err and stable_clock as _mk (release[a] may
 * be the step of a StableAtShard event); a failing event leaves no trace and
 * the rows of earlier events stay valid.  stable_sent: NULL, or a plane:
 * stable_sent[a] = the step during which the partial of attached event a made
 * its command stable at this shard, i.e. ran send_stable_msg (:296-309, called
 * at :314 and :331); rows of every other event are not written (fill with
 * FX_RELEASE_NONE).  For a command entirely at one shard this marks the _mk
 * sender; a single-key command at one shard sends nothing and has no row.
 * Every other (shard, key) of the command is owed one StableAtShard per row.
 *
 * The _mk input check on the events of one dot gains "same shards"; an op that
 * sent counts as told.
 *
 * Capacities per stream: live ops, to_executors and vote windows as _mk;
 * buffered (key, rifl) pairs -- common here: a message from a fast shard often
 * beats local stability -- FX_TABLE_PS_ONCHIP_BUFFERED / FX_TABLE_PS_HBM_BUFFERED
 * (registers on chip; on the HBM tier in `state`, whose size is
 * fx_table_state_bytes_ps; fx_table_state_bytes is unchanged).  Beyond a
 * limit the stream stops with FX_ERR_CAPACITY and fx_table_run_ps reruns it
 * whole on the HBM tier. */
#define FX_TABLE_MAX_CMD_SHARDS 8u
#define FX_TABLE_PS_ONCHIP_BUFFERED 64u
#define FX_TABLE_PS_HBM_BUFFERED 512u
#define FX_TABLE_PS_WORD(nkeys, shards) ((uint32_t)(nkeys) | ((uint32_t)(shards) << 8))
#define FX_TABLE_PS_WORD_NKEYS(w) ((uint32_t)(w) & 0xFFu)
#define FX_TABLE_PS_WORD_SHARDS(w) ((uint32_t)(w) >> 8)
#define FX_TABLE_HDR_STABLE(key) FX_TABLE_HDR(FX_TABLE_DETACHED, 127u, key)
/* As fx_table_execute_mk / fx_table_run_mk plus stable_sent (same profile
 * slots; `state` of the HBM tier: fx_table_state_bytes_ps). */
size_t fx_table_state_bytes_ps(uint32_t n, uint32_t keys, uint32_t lanes);
int fx_table_execute_ps(const fx_table_batch_mk* in, const fx_order_batch* out, uint32_t* stable_clock,
                        uint32_t* stable_sent, const uint32_t* stream_map, uint32_t num_lanes, uint32_t tier,
                        void* state, uint32_t flags, void* hip_stream);
int fx_table_run_ps(const fx_table_batch_mk* in, const fx_order_batch* out, uint32_t* stable_clock,
                    uint32_t* stable_sent, uint32_t flags, void* hip_stream, uint32_t* reruns);

/* Resumable streams: the table executor fed in pieces.  fx_table_advance runs
 * rows [done, len) of every stream -- len = lengths[s] or steps, done = where
 * the stream's previous call stopped (0 with FX_FLAG_INIT, which starts the
 * stream from an empty executor whatever `state` holds) -- on the HBM-tier
 * tables with the semantics of fx_table_execute (FX_TABLE_KIND_SINGLE; nkeys
 * may be NULL), fx_table_execute_mk (_MK) or fx_table_execute_ps (_PS;
 * stable_sent NULL or a plane, NULL for the other kinds).  The outputs are
 * the planes of those entry points and are cumulative: arrival indices are
 * plane rows, order row k is the k-th executed partial since row 0, nexec the
 * running total, stable_clock is written after every call's last handled
 * event.  For any partition of [0, L) into calls every output is bit-identical
 * to one whole-stream call at FX_TABLE_TIER_HBM over the same planes.  Rows
 * below done are not read again; rows at or above len may hold anything.
 *   len == done  nothing but the state header is read; err[s] and nexec[s]
 *                are rewritten with their current values
 *   len < done   FX_ERR_INVALID_ARG for the stream, state as it was
 * steps, n, keys, vmax, stability_threshold, kind and
 * FX_FLAG_EXECUTE_AT_COMMIT are fixed for a session: the kernel keeps them in
 * the state and a call that differs stops the stream with FX_ERR_INVALID_ARG,
 * state as it was.  A stream that stopped with an error stays stopped: later
 * calls handle nothing for it and report the same status.  FX_ERR_CAPACITY is
 * final (there is no tier above).  What a call's last event left on
 * to_executors for the next event's drain waits in `state`.
 * state: fx_table_session_bytes(kind, n, keys, num_streams) bytes, indexed by
 * stream (no stream_map).  flags: FX_FLAG_INIT, FX_FLAG_EXECUTE_AT_COMMIT.
 * Asynchronous; profile slot FX_PROFILE_SLOT_TABLE + 2.  The ONCHIP tier is
 * not offered: it keeps its tables in LDS and registers. */
#define FX_TABLE_KIND_SINGLE 0u
#define FX_TABLE_KIND_MK 1u
#define FX_TABLE_KIND_PS 2u
size_t fx_table_session_bytes(uint32_t kind, uint32_t n, uint32_t keys, uint32_t num_streams);
int fx_table_advance(const fx_table_batch_mk* in, uint32_t kind, const fx_order_batch* out, uint32_t* stable_clock,
                     uint32_t* stable_sent, void* state, uint32_t flags, void* hip_stream);

/* Closed-loop shard groups: the shard executors of a group run together and
 * the StableAtShard messages one of them sends reach the others inside the
 * kernel.  One workgroup per group, one wavefront per shard executor; the
 * input is each shard's own events and nothing else, the whole loop is one
 * launch (what fantoch_amd.table.run_table_groups paces from the host).
 *
 * Inputs: `own` holds the own events of num_streams = groups * shards streams
 * (attached / detached, nkeys words FX_TABLE_PS_WORD; stream g * shards + h is
 * shard h of group g).  `route` is a plane over own's rows: for the attached
 * event of a command with shards > 1, the index i into `targets` of the list
 * of the command's keys at the other shards -- targets[i] = m, then m words
 * FX_TABLE_TARGET(delay, shard, key), in delivery order; the events of one
 * command at one shard may share a list.  Other rows are ignored.
 *
 * Rounds: in round t = 0, 1, ... every shard first handles
 * the messages of its inbox that are due at or before t, ascending by (due
 * round, send index), then its own event t if it has one.  Every handled
 * event takes the next row j of the stream's handled sequence: the step, the
 * arrival indices in `order`, and the rows of `release` and `stable_sent`
 * count in those rows, and handled_src / handled_dot say what row j was (an
 * own row, or FX_TABLE_HANDLED_MSG | key with the message's rifl).  Each
 * event is handled with the semantics of fx_table_execute_ps at
 * FX_TABLE_TIER_HBM (512 live ops, 512 to_executors entries, 512 buffered
 * pairs), its drain included.
 * Sends: a try that runs send_stable_msg for a command with shards > 1 writes
 * stable_sent[j] and sends.  After round t the sends of the group are taken
 * over its shards ascending, per shard ascending by (step, handled row); each
 * send's target list is walked in order and every message takes the group's
 * next send index, whether or not it is kept; the message (key, rifl) for
 * shard h is due at round t + 1 + delay.
 * A stream that stops with an error handles nothing more, messages to it are
 * dropped, and the other shards of its group go on; the events the round still
 * held for it are listed in handled_src / handled_dot (as the host-paced loop
 * lists them) but not handled.  A group ends when no shard of it has own
 * events or undelivered messages left; rounds[g] counts its rounds.  The
 * rounds of a call are capped at own.steps + 33 * shards * steps_out + 1,
 * which well-formed inputs cannot reach; at the cap every unfinished stream
 * stops with FX_ERR_INVALID_ARG.
 *
 * Input check, before round 0: a stream with a FX_TABLE_HDR_STABLE event among
 * its own events, or with an attached event of shards > 1 whose route is
 * FX_TABLE_ROUTE_NONE, reaches (with its list) beyond targets_words, names a
 * shard >= shards or its own shard or a key >= keys, or whose list's shards do
 * not number shards - 1, never starts: FX_ERR_INVALID_ARG, nexec 0.
 *
 * Capacities per stream, beside those of fx_table_execute_ps at the HBM tier:
 * FX_TABLE_GROUP_INBOX undelivered messages (beyond: FX_ERR_CAPACITY when the
 * message is sent, the stream stops after the round's events), and
 * FX_TABLE_GROUP_SENDS sends per round (FX_ERR_CAPACITY at the try that would
 * send, before anything of that try is written); more handled events than
 * steps_out rows is FX_ERR_ORDER_OVERFLOW.  Per group 5,128 bytes of LDS per
 * shard.
 *
 * Outputs: planes of steps_out rows over the handled rows.  release and
 * stable_sent rows below handled_len are always written (FX_RELEASE_NONE
 * where fx_table_execute_ps writes nothing); rows at and above it are not.
 * state: fx_table_groups_state_bytes bytes, contents ignored.
 * Argument errors (a null pointer but stable_clock, shards outside
 * 1..FX_TABLE_MAX_CMD_SHARDS, num_streams no multiple of shards, steps or
 * steps_out of 0 or >= 2^26, the limits of fx_table_execute_ps) are returned
 * before any launch.  flags: FX_FLAG_EXECUTE_AT_COMMIT.  Asynchronous;
 * profile slot FX_PROFILE_SLOT_TABLE + 3. */
#define FX_TABLE_GROUP_MAX_DELAY 31u
#define FX_TABLE_GROUP_INBOX 256u
#define FX_TABLE_GROUP_SENDS 64u
#define FX_TABLE_ROUTE_NONE 0xFFFFFFFFu
#define FX_TABLE_TARGET(delay, shard, key) \
  (((uint32_t)(delay) << 27) | (((uint32_t)(shard) & 7u) << 24) | ((uint32_t)(key) & 0x00FFFFFFu))
#define FX_TABLE_HANDLED_MSG 0x80000000u /* handled_src: a routed message; low 24 bits = key */
typedef struct fx_table_group_batch {
  fx_table_batch_mk own;     /* own events only; num_streams = groups * shards            */
  const uint32_t* route;     /* plane over own's rows: index into targets, or ignored     */
  const uint32_t* targets;   /* lists: m, then m words FX_TABLE_TARGET                    */
  uint32_t targets_words;
  uint32_t shards;           /* P, 1..FX_TABLE_MAX_CMD_SHARDS                             */
  uint32_t steps_out;        /* rows of every output plane                                */
} fx_table_group_batch;
typedef struct fx_table_group_out {
  fx_order_batch out;        /* order, release, nexec, err over handled rows              */
  uint32_t* stable_clock;    /* NULL or [S * keys]                                        */
  uint32_t* stable_sent;     /* plane, handled rows                                       */
  uint32_t* handled_src;     /* plane: own row index, or FX_TABLE_HANDLED_MSG | key       */
  uint32_t* handled_dot;     /* plane: the rifl of a routed message (0 for own events)    */
  uint32_t* handled_len;     /* [S] handled rows, the failing event included              */
  uint32_t* rounds;          /* [groups] rounds the group ran                             */
} fx_table_group_out;
size_t fx_table_groups_state_bytes(uint32_t n, uint32_t keys, uint32_t num_streams);
int fx_table_run_groups(const fx_table_group_batch* in, const fx_table_group_out* out, void* state, uint32_t flags,
                        void* hip_stream);
/* Config::tempo_quorum_sizes (fantoch/src/config.rs:337-349): fast quorum
 * minority + f (2f with tiny quorums), write quorum f + 1, stability
 * threshold minority + 1 (n - f with tiny quorums). */
int fx_tempo_quorum_sizes(uint32_t n, uint32_t f, uint32_t tiny, uint32_t* fast_quorum, uint32_t* write_quorum,
                          uint32_t* stability_threshold);

/* --------------------------------------- synthetic Atlas/EPaxos streams */
/* Commit streams of `instances` independent simulated instances; instance i
 * has n processes, each coordinating cmds_per_process commands; conflict rate
 * conflict_pct[i % num_conflicts] percent (fantoch/src/client/key_gen.rs:96-128
 * semantics with a counter-based RNG, canonical C6); delivery order per process is a
 * seeded windowed shuffle; concurrent same-key commands of the same round see
 * each other with probability cycle_pct (2-/k-cycles). */
typedef struct fx_synth_params {
  uint64_t seed;
  uint32_t instances;
  uint32_t instance_base;    /* global index of the first instance (multi-GPU) */
  uint32_t n;
  uint32_t cmds_per_process;
  uint32_t window;           /* delivery jitter window (generation units)   */
  uint32_t cycle_pct;
  uint32_t horizon;          /* rounds searched back for the latest conflict */
  uint32_t num_conflicts;
  uint32_t conflict_pct[8];
  uint32_t conflict_block;   /* 0: rate = conflict_pct[i % num_conflicts] (seed-major);
                                B: rate = conflict_pct[(i / B) % num_conflicts]
                                (conflict-major: B consecutive instances share a rate) */
  uint32_t clients;          /* closed-loop clients per process (0/1: one; C >= 2:
                                seqs form rounds of C concurrent commands per source,
                                a command sees other sources' earlier rounds only, and
                                with probability cycle_pct a random concurrent command
                                of any other source: large SCCs, BASELINE configs[3];
                                cmds_per_process must be a multiple of C)            */
  uint32_t key_pool;         /* 0: the conflict-key model above.  K >= 2 (one client
                                per process): SURVEY §8(d)'s S5 stream, per-key chains
                                over a pool of K keys: every command's key is a C6
                                draw from the pool, its deps are, per source, the
                                latest command on that key within `horizon` rounds
                                (its own source: earlier seqs only), and with
                                probability cycle_pct two commands of the same round
                                depend on each other (2-cycles; longer cycles through
                                the chains).  conflict_pct is not used.              */
} fx_synth_params;

/* Planes of the synthetic batch: S = instances * n, steps = n * cmds, dmax = n. */
int fx_synth_shape(const fx_synth_params* p, uint32_t* num_streams, uint32_t* steps, uint32_t* dmax);
/* Generate into device planes (dot/hdr/deps of `out`, caller allocated). */
int fx_synth_generate(const fx_synth_params* p, uint32_t* dot, uint32_t* hdr, uint32_t* deps, void* hip_stream);
/* Same generator on the host (identical bytes). */
int fx_synth_generate_host(const fx_synth_params* p, uint32_t* dot, uint32_t* hdr, uint32_t* deps);

/* ------------------------------------------ synthetic Caesar commit streams */
/* Seeded commit streams for the predecessors executor (fx_pred_batch), in the
 * shape of Caesar's own commits; the model is stated once, for host and
 * device, in fantoch_amd/csrc/fx_pred_synth.h.  Per
 * instance of n processes with one closed-loop client each, command
 * g = (round j, coordinator s) has dot (s, j) and fx_synth's key (the shared
 * key with probability conflict_pct, else the coordinator's own).  With
 * K = max_bump + 1 its proposal clock is (K j, s).  A command on the shared
 * key is retried with probability retry_pct (max_bump > 0) with a bump r in
 * 1..max_bump, capped at the rounds left; its final, committed clock is
 * (K (j + r) + r, s), r = 0 without a retry.  Its deps are what
 * KeyClocks::predecessors answers at the quorum when it gets that clock:
 * every other command on its key of a round >= j - horizon whose proposal
 * clock is lower than its final clock -- rounds [j - horizon, j) and the lower
 * sources of round j, with a bump r every round through j + r.  Delivery is
 * fx_synth's (arrival keys and windowed ranks); the header's deps field holds
 * min(ndeps, 31), the ndeps plane the count.
 * Shape: S = instances * n, steps = n * cmds_per_process,
 * dmax = n * (horizon + max_bump + 1) - 1.
 * Refused with FX_ERR_INVALID_ARG before any launch or store: a null params
 * or planes, dmax > FX_PRED_MAX_DEPS, n outside 1..8, cmds_per_process == 0,
 * instances == 0, retry_pct > 100, num_conflicts > 8, steps + window >= 2^24,
 * instance_base + instances or instances * n beyond 32 bits, a null plane
 * (ndeps may be NULL when dmax <= 31). */
typedef struct fx_pred_synth_params {
  uint64_t seed;
  uint32_t instances;
  uint32_t instance_base;    /* global index of the first instance               */
  uint32_t n;
  uint32_t cmds_per_process;
  uint32_t window;           /* delivery jitter window, as fx_synth_params        */
  uint32_t horizon;          /* rounds of history a command's deps reach back (the
                                GC of the key clocks)                             */
  uint32_t max_bump;         /* largest number of rounds a retry moves a clock    */
  uint32_t retry_pct;        /* chance that a shared-key command is retried       */
  uint32_t num_conflicts;
  uint32_t conflict_pct[8];  /* as fx_synth_params                                */
  uint32_t conflict_block;   /* as fx_synth_params.conflict_block                 */
} fx_pred_synth_params;
/* The planes of an fx_pred_batch: dot, hdr, clock_lo, clock_hi and ndeps of
 * fx_plane_words(S, steps) words, deps of dmax such planes. */
typedef struct fx_pred_synth_planes {
  uint32_t *dot, *hdr, *deps, *clock_lo, *clock_hi, *ndeps;
} fx_pred_synth_planes;
int fx_pred_synth_shape(const fx_pred_synth_params* p, uint32_t* num_streams, uint32_t* steps, uint32_t* dmax);
/* Generate into device planes.  Every word of rows < steps of streams < S is
 * written in every plane, the unused slots of all dmax dep planes as 0; pad
 * rows and pad streams are not touched.  Asynchronous on hip_stream. */
int fx_pred_synth_generate(const fx_pred_synth_params* p, const fx_pred_synth_planes* planes, void* hip_stream);
/* The same on the host (identical bytes).  No device needed. */
int fx_pred_synth_generate_host(const fx_pred_synth_params* p, const fx_pred_synth_planes* planes);
/* Measurement only: fx_pred_synth_generate with a named form of the kernel
 * (the same bytes): 0 = a workgroup per tile of commands, flags and jitters
 * drawn once into LDS; 1 = one thread per command, the host twin's loop, which
 * is what fx_pred_synth_generate runs (the tile form measured no faster). */
#define FX_PRED_SYNTH_FORM_TILE 0u
#define FX_PRED_SYNTH_FORM_COMMAND 1u
int fx_pred_synth_generate_form(const fx_pred_synth_params* p, const fx_pred_synth_planes* planes, uint32_t form,
                                void* hip_stream);

/* ------------------------------------------- synthetic Tempo vote streams */
/* Seeded streams of TableExecutionInfo values for fx_table_run / fx_table_run_mk,
 * generated on the device into the planes of an fx_table_batch_mk (or on the
 * host: the same bytes).  Stream s of a call is global stream stream_base + s;
 * every draw is the counter RNG of fx_synth (canonical C6) keyed by (seed,
 * global stream, command index, purpose), so a stream does not depend on the
 * launch it is part of.  Per stream, n processes keep a clock per key
 * (SequentialKeyClocks, fantoch_ps/src/protocol/common/table/clocks/keys/
 * sequential.rs:38-114).  Command i has 1..min(kmax, keys) keys: the first is
 * key 0 with probability conflict percent, else a uniform other key, the
 * further ones distinct uniform other keys; a uniform coordinator and
 * fast_quorum - 1 distinct other processes form its fast quorum.  The
 * coordinator proposes its highest clock over the command's keys plus one,
 * every other member the higher of that and its own highest plus one; each
 * votes own + 1 .. its proposal on every key; the commit clock is the highest
 * proposal; the dot is (coordinator, its command count).  Events: one
 * AttachedVotes per key (ascending key id, votes coordinator first, then the
 * members as picked, `nkeys` = the command's key count; tempo.rs:614-636), all
 * delivered in slot i + U[0, window]; then per key and process below the
 * commit clock one DetachedVotes own + 1 .. commit, in slot i + U[0, lag] of
 * its own.  A stream is its events by (slot, creation order).  The model and
 * the numbering of the draws: fantoch_amd/csrc/fx_table_synth.h.
 * conflict rate of global stream g: conflict_pct[g % num_conflicts]
 * (conflict_block 0) or conflict_pct[(g / conflict_block) % num_conflicts], as
 * fx_synth_params.
 * Accepted: 1 <= n <= 16, 1 <= fast_quorum <= n, 1 <= kmax <=
 * FX_TABLE_MAX_CMD_KEYS, 1 <= keys <= FX_TABLE_SYNTH_MAX_KEYS, cmds, window and
 * lag <= FX_SEQ_MASK, num_conflicts <= 8 (0 counts as 1), every rate in use <=
 * 100, stream_base + streams <= 2^32, cmds * min(kmax, keys) * n below 2^32;
 * anything else is FX_ERR_INVALID_ARG with nothing written. */
#define FX_TABLE_SYNTH_MAX_KEYS (1u << 16)
/* Per-stream state is (keys + 1) * n words (the clocks and the coordinators'
 * command counts); up to this many words it lives in LDS (64 streams of a
 * wavefront: 64 KiB), above in the scratch buffer. */
#define FX_TABLE_SYNTH_ONCHIP_WORDS 256u
typedef struct fx_table_synth_params {
  uint64_t seed;
  uint32_t streams;
  uint32_t stream_base;      /* global index of the first stream (multi-GPU) */
  uint32_t n;
  uint32_t fast_quorum;
  uint32_t keys;
  uint32_t cmds;             /* commands per stream                          */
  uint32_t kmax;             /* keys per command 1..min(kmax, keys)          */
  uint32_t window;           /* attached events up to this many commands late */
  uint32_t lag;              /* detached events up to this many commands late */
  uint32_t num_conflicts;
  uint32_t conflict_pct[8];
  uint32_t conflict_block;   /* as fx_synth_params.conflict_block            */
} fx_table_synth_params;
/* The planes of an fx_table_batch_mk, writable: hdr / dot / clock / nkeys of
 * fx_plane_words(streams, steps) words, votes of 3 * fast_quorum such planes,
 * lengths[streams].  nkeys may be NULL when kmax == 1. */
typedef struct fx_table_synth_planes {
  uint32_t* hdr;
  uint32_t* dot;
  uint32_t* clock;
  uint32_t* votes;
  uint32_t* nkeys;
  uint32_t* lengths;
} fx_table_synth_planes;
/* *max_steps = cmds * min(kmax, keys) * n, which no stream exceeds (a command
 * makes at most K attached and K (n - 1) detached events: the member with the
 * highest proposal is at the commit clock already); *vmax = fast_quorum.  Host
 * only. */
int fx_table_synth_shape(const fx_table_synth_params* p, uint32_t* max_steps, uint32_t* vmax);
/* Bytes of device scratch the device entry points need (0: bad arguments):
 * one counter per (delivery slot, stream) and, beyond
 * FX_TABLE_SYNTH_ONCHIP_WORDS, the per-stream state. */
size_t fx_table_synth_scratch_bytes(const fx_table_synth_params* p);
/* The counting pass: lengths_dev[s] = events of stream s; *max_len (optional)
 * = the longest.  Synchronous. */
int fx_table_synth_lengths(const fx_table_synth_params* p, uint32_t* lengths_dev, void* scratch, void* hip_stream,
                           uint32_t* max_len);
/* Counts (as fx_table_synth_lengths, into planes->lengths), returns
 * FX_ERR_CAPACITY before any plane store if a stream is longer than `steps`,
 * else writes every stream; rows at or past a stream's length and the pad
 * streams of the last tile are 0 in every plane, so every word of
 * fx_plane_words(streams, steps) per plane is defined and none beyond is
 * touched.  The planes are ready when the call returns on `hip_stream` order
 * (the kernels are queued, the counting pass has been waited for). */
int fx_table_synth_generate(const fx_table_synth_params* p, const fx_table_synth_planes* planes, uint32_t steps,
                            void* scratch, void* hip_stream);
/* The same on the host (identical bytes; FX_ERR_CAPACITY likewise), and the
 * counting pass alone.  No device needed. */
int fx_table_synth_generate_host(const fx_table_synth_params* p, const fx_table_synth_planes* planes, uint32_t steps);
int fx_table_synth_lengths_host(const fx_table_synth_params* p, uint32_t* lengths, uint32_t* max_len);

/* ------------------------------------------ synthetic closed-loop shard groups */
/* Seeded input of fx_table_run_groups, generated on the device (or on the
 * host: the same bytes): the own events of groups * shards streams in the
 * planes of an fx_table_batch_mk, the route plane, the targets array and the
 * lengths.  Group j of a call is global group G = group_base + j; stream
 * j * shards + h is its shard h.  Every draw is the counter RNG of fx_synth
 * (canonical C6) as synth_rand(seed, G, a, purpose), so a group does not
 * depend on the launch it is part of.  Every shard of a group has its own n
 * processes with a clock per key.  Command i = 0 .. cmds-1 of the group:
 *   shard set    1 + draw % min(smax, shards) shards, distinct, uniform
 *   coordinator  one process p for the command; dot (p, its command count over
 *                the group)
 *   per shard h  1..min(kmax, keys) keys, coordinator p and fast_quorum - 1
 *                other processes, proposals and votes over that shard's clocks:
 *                all as command i of fx_table_synth_params
 *   commit       the highest proposal over all the command's shards
 *                (fantoch_ps/src/protocol/tempo.rs:614-636)
 *   events at h  one AttachedVotes per key (ascending; the commit clock, the
 *                key's votes, nkeys word FX_TABLE_PS_WORD(keys at h, shards of
 *                the command)), all in slot i + U[0, window] drawn per shard;
 *                then per key and process below the commit clock at h one
 *                DetachedVotes own + 1 .. commit in slot i + U[0, lag]
 *   route        for a command at more than one shard, each of its shards h
 *                has one list in targets: m, then m words FX_TABLE_TARGET(delay,
 *                shard, key) over the command's keys at its other shards,
 *                ascending by (shard, key), delay = U[0, msg_lag] drawn per
 *                (h, command, target shard, key index); the command's attached
 *                events at h hold the list's index in `route`, every other row
 *                FX_TABLE_ROUTE_NONE.
 * A stream is its events by (slot, creation order); the lists of a group
 * follow each other by (shard, slot of the attached events, command), the
 * groups' lists in group order -- the arrays of
 * fantoch_amd.table.pack_table_groups, but for the nkeys plane on rows that
 * hold no attached event: 0 here, as in every plane (the packer stores the
 * word of a one-key, one-shard command there; the executor does not read it).  The numbering of the draws (group
 * level a = i, per shard a = i | (h + 1) << 32):
 * fantoch_amd/csrc/fx_table_group_synth.h.
 * conflict rate of group G: conflict_pct[G % num_conflicts] (conflict_block 0)
 * or conflict_pct[(G / conflict_block) % num_conflicts].
 * Accepted: the limits of fx_table_synth_params on n, fast_quorum, keys, kmax,
 * cmds, window, lag and the rates; 1 <= shards, smax <= FX_TABLE_MAX_CMD_SHARDS;
 * msg_lag <= FX_TABLE_GROUP_MAX_DELAY; (group_base + groups) * shards <= 2^32
 * and groups * shards < 2^32 (a batch's num_streams); *max_steps_out of
 * fx_table_group_synth_shape below 2^26 (fx_table_run_groups' limit on rows),
 * and with it the words of one group's lists below 2^32; anything else is
 * FX_ERR_INVALID_ARG, nothing written. */
typedef struct fx_table_group_synth_params {
  uint64_t seed;
  uint32_t groups;
  uint32_t group_base;       /* global index of the first group (multi-GPU)  */
  uint32_t shards;           /* P: shard executors per group                 */
  uint32_t smax;             /* shards per command 1..min(smax, shards)      */
  uint32_t n;
  uint32_t fast_quorum;
  uint32_t keys;             /* per shard                                    */
  uint32_t cmds;             /* commands per group                           */
  uint32_t kmax;             /* keys per command and shard 1..min(kmax, keys) */
  uint32_t window;
  uint32_t lag;
  uint32_t msg_lag;          /* StableAtShard messages up to this many rounds late */
  uint32_t num_conflicts;
  uint32_t conflict_pct[8];
  uint32_t conflict_block;
} fx_table_group_synth_params;
/* The planes of an fx_table_batch_mk, writable, over groups * shards streams
 * (votes: 3 * fast_quorum planes), the route plane, targets and
 * lengths[groups * shards].  targets may be NULL while targets_words is 0. */
typedef struct fx_table_group_synth_planes {
  uint32_t* hdr;
  uint32_t* dot;
  uint32_t* clock;
  uint32_t* votes;
  uint32_t* nkeys;
  uint32_t* route;
  uint32_t* targets;
  uint32_t* lengths;
} fx_table_group_synth_planes;
/* Upper bounds, with kcap = min(kmax, keys) and scap = min(smax, shards).
 * *max_steps: rows no stream's own events exceed, cmds * kcap * n when
 * scap == 1 (as fx_table_synth_shape) and cmds * kcap * (n + 1) otherwise: a
 * key of a command has one attached event and one detached event per process
 * below the commit clock, and where that clock comes from another shard all n
 * processes are below it.  *max_steps_out: the same of the handled rows, one
 * StableAtShard per key and other shard of the command on top: cmds * kcap *
 * (n + scap) when scap > 1; at least 1.  *vmax = fast_quorum.
 * *max_targets_words: words the lists of one group cannot exceed, cmds * scap
 * * (1 + kcap * (scap - 1)) when scap > 1, else 0.  Host only. */
int fx_table_group_synth_shape(const fx_table_group_synth_params* p, uint32_t* max_steps, uint32_t* max_steps_out,
                               uint32_t* vmax, uint64_t* max_targets_words);
/* Bytes of device scratch the device entry points need (0: bad arguments):
 * per group two counters per (shard, delivery slot), a few words per shard
 * and, beyond FX_TABLE_SYNTH_ONCHIP_WORDS, the state (shards * keys * n + n
 * words: the clocks and the coordinators' command counts). */
size_t fx_table_group_synth_scratch_bytes(const fx_table_group_synth_params* p);
/* The counting pass: lengths_dev[s] = own events of stream s; *max_len = the
 * longest; *steps_out = the rows fx_table_run_groups needs per output plane
 * (the highest over the streams of own events + keys here * other shards per
 * command that spans shards; at least 1); *targets_words = the words of all
 * lists (the three optional).  Synchronous. */
int fx_table_group_synth_count(const fx_table_group_synth_params* p, uint32_t* lengths_dev, void* scratch,
                               void* hip_stream, uint32_t* max_len, uint32_t* steps_out, uint64_t* targets_words);
/* Counts, returns FX_ERR_CAPACITY before any store to the caller's buffers
 * (the lengths included) if a stream is longer than `steps` or the lists need
 * more than targets_words words, else writes every group: rows at or past a stream's
 * length and the pad streams of the last tile are 0 in every plane and
 * FX_TABLE_ROUTE_NONE in route; no word beyond fx_plane_words(groups * shards,
 * steps) per plane is touched, and of targets exactly the words the lists
 * take.  Ready on `hip_stream` order when the call returns. */
int fx_table_group_synth_generate(const fx_table_group_synth_params* p, const fx_table_group_synth_planes* planes,
                                  uint32_t steps, uint32_t targets_words, void* scratch, void* hip_stream);
/* The same on the host (identical bytes), and the counting pass alone.  No
 * device needed. */
int fx_table_group_synth_generate_host(const fx_table_group_synth_params* p,
                                       const fx_table_group_synth_planes* planes, uint32_t steps,
                                       uint32_t targets_words);
int fx_table_group_synth_count_host(const fx_table_group_synth_params* p, uint32_t* lengths, uint32_t* max_len,
                                    uint32_t* steps_out, uint64_t* targets_words);

/* ------------------------------------- KVStore results and per-key monitors */
/* The last step of every executor: Command::execute -> KVStore::execute ->
 * ExecutionOrderMonitor::add (fantoch/src/command.rs:147-162, kvs.rs:53-85,
 * executor/monitor.rs:8-55), for a batch, from the order plane any batched
 * engine wrote.  Canonical C15: a value is a u32 id in 1 .. 2^30 - 1 and 0 is
 * None; interning the strings is the caller's job, as for keys (C7).  An op is
 * one word, a partial (Vec<KVOp>, all on one key) up to omax of them in slot
 * order:
 *   Get     returns the current value
 *   Put(v)  stores v and returns None (not the previous value, kvs.rs:77-80)
 *   Delete  removes the key and returns the removed value
 * A partial is read-only if every op is a Get (kvs.rs:61; an empty one is, and
 * has no results); the monitor skips read-only partials (monitor.rs:22-24). */
#define FX_KV_GET 0u
#define FX_KV_PUT 1u
#define FX_KV_DELETE 2u
#define FX_KV_EMPTY 3u            /* unused op slot */
#define FX_KV_OP(kind, value) ((((uint32_t)(kind) & 3u) << 30) | ((uint32_t)(value) & 0x3FFFFFFFu))
#define FX_KV_OP_KIND(op) ((uint32_t)(op) >> 30)
#define FX_KV_OP_VALUE(op) ((uint32_t)(op) & 0x3FFFFFFFu)
#define FX_KV_MAX_OPS 4u
#define FX_KV_AGREE 0xFFFFFFFFu
#define FX_KV_BAD_PAIR 0xFFFFFFFEu /* fx_kv_monitor_compare: a pair that cannot be compared */
/* The value and the monitor cursor of every key of a stream (2 words per key)
 * live in LDS up to this many keys, above in the stream's own store / mon_off
 * rows.  One wavefront per stream and workgroup: a CU holds at most 32 such
 * workgroups, and 32 x 2 x 512 x 4 B = 128 KiB of its 160 KiB of LDS, so LDS
 * never lowers the occupancy. */
#define FX_KV_ONCHIP_KEYS 512u
typedef struct fx_kv_batch {
  const uint32_t* order;   /* plane of an fx_order_batch (row k: arrival row | maybe FX_ORDER_SCC_START) */
  const uint32_t* nexec;   /* [S] rows of `order` to execute                                           */
  const uint32_t* key;     /* plane by arrival row; the key is (word & key_mask)                       */
  uint32_t key_mask;       /* 0x00FFFFFF lets a table `hdr` plane be passed as it is                   */
  const uint32_t* ops;     /* omax planes by arrival row, slot j = plane j; used slots first           */
  uint32_t num_streams, steps, keys, omax;
} fx_kv_batch;
typedef struct fx_kv_out {
  uint32_t* result;   /* omax planes by arrival row: result of slot j (0 = None; 0 in the unused
                         slots of an executed row); rows that were not executed: untouched           */
  uint32_t* store;    /* [S * keys] final value per key, 0 = absent                                    */
  uint32_t* monitor;  /* plane: rows mon_off[k] .. mon_off[k+1]-1 = arrival rows of the write partials
                         executed on key k, in execution order; rows from mon_off[keys] on: untouched  */
  uint32_t* mon_off;  /* [S * (keys + 1)]                                                              */
  uint32_t* err;      /* [S]                                                                           */
} fx_kv_out;
/* Executes, per stream, the partials of the first nexec rows of `order` in
 * that order.  Per-stream status, decided before anything else of the stream
 * is stored: nexec > steps is FX_ERR_ORDER_OVERFLOW; an arrival row >= steps,
 * a key >= keys, a PUT of value 0 or a used slot after an EMPTY one is
 * FX_ERR_INVALID_ARG; such a stream writes its err only.  An arrival row is
 * expected at most once among a stream's nexec rows (what every executor
 * writes); the result words of one that repeats are those of one of its
 * executions.  Refused with FX_ERR_INVALID_ARG and nothing written: a null
 * pointer, omax outside 1..FX_KV_MAX_OPS, keys outside 1..FX_TABLE_MAX_KEYS.
 * Device pointers; asynchronous on hip_stream.  Order, key and op planes hold
 * fx_plane_words(num_streams, steps) words each. */
int fx_kv_execute(const fx_kv_batch* in, const fx_kv_out* out, void* hip_stream);
/* The same on the host (host pointers, identical bytes).  No device needed. */
int fx_kv_execute_host(const fx_kv_batch* in, const fx_kv_out* out);

/* Resumable streams: the KV stage fed in pieces, behind an executor session
 * (fx_table_advance, fx_slot_advance, fx_pred_advance).  `in` is
 * fx_kv_execute's batch over the executor's cumulative order plane.  A call
 * executes order rows [done, nexec[s]) of every stream; done = where the
 * stream's previous call stopped (0 with FX_FLAG_INIT, which starts from an
 * empty store whatever `state` holds).  Rows below done must not have changed
 * since they were consumed (every executor session guarantees it) and are not
 * read again.  Between calls the store lives in `state`: per stream a header
 * {tag, steps, keys, omax, done, err}, the value of every key and the number
 * of write partials executed on every key so far.
 * After every call of a partition in which every nexec[s] <= steps does not
 * decrease and no row is invalid, every word of result and store equals what
 * one fx_kv_execute over the same planes with this call's nexec leaves on
 * buffers of the same initial content.  rank[a] of an executed write partial
 * is its index in its key's sequence (its monitor row less the key's first
 * row); fx_kv_session_monitor lays the CSR monitor out from it on demand.
 *   a call with FX_FLAG_INIT that does not fail writes the stream's store row
 *                   whatever nexec[s] is (0: an empty store)
 *   nexec == done   err[s] is rewritten and nothing else
 *   nexec < done    err[s] = FX_ERR_INVALID_ARG for this call, state as it was
 *   nexec > steps   err[s] = FX_ERR_ORDER_OVERFLOW for this call, state as it
 *                   was (with FX_FLAG_INIT: an empty store with done = 0)
 *   an invalid row  (fx_kv_execute's checks) among the call's own rows: the
 *                   stream stops with FX_ERR_INVALID_ARG before the call stores
 *                   a word of it; what earlier calls wrote stands; later calls
 *                   rewrite err[s] with that status and nothing else
 * steps, keys and omax are fixed for a session.  A wrong tag (a state that
 * never saw FX_FLAG_INIT), or other steps, keys or omax than the header holds:
 * err[s] = FX_ERR_INVALID_ARG and nothing else of the stream read or written.
 * Refused with FX_ERR_INVALID_ARG before any launch: what fx_kv_execute
 * refuses, a null state or rank, flags other than FX_FLAG_INIT.
 * state: fx_kv_session_bytes(keys, num_streams) bytes, indexed by stream; it
 * belongs to the side (device or host) that initialised it.  Asynchronous. */
typedef struct fx_kv_session_out {
  uint32_t* result;  /* omax planes by arrival row, cumulative, as fx_kv_out.result                  */
  uint32_t* store;   /* [S * keys] the store after the rows consumed so far; written by every
                        call that consumes a row (and by one with FX_FLAG_INIT that consumes none)   */
  uint32_t* rank;    /* plane by arrival row: an executed write partial's index among the write
                        partials of its key; other rows: untouched                                   */
  uint32_t* err;     /* [S]                                                                          */
} fx_kv_session_out;
size_t fx_kv_session_bytes(uint32_t keys, uint32_t num_streams);
int fx_kv_advance(const fx_kv_batch* in, const fx_kv_session_out* out, void* state, uint32_t flags,
                  void* hip_stream);
/* The same on the host (host pointers, a state of its own): the same output
 * and state bytes for the same sequence of calls.  No device needed. */
int fx_kv_advance_host(const fx_kv_batch* in, const fx_kv_session_out* out, void* state, uint32_t flags);
/* The monitor of the rows a session has consumed, built on demand (a CSR
 * cannot be laid out before the counts are final).  `in` as in the session's
 * calls (nexec is not read: done comes from the state), rank the session's
 * rank plane.  Writes mon_off = the exclusive prefix of the state's counts,
 * monitor[mon_off[key] + rank[a]] = a for every consumed write row, store
 * from the state and err = the stream's status: after a session of valid rows
 * the bytes fx_kv_execute over the consumed rows leaves in monitor, mon_off,
 * store and err (out->result is not written); after a stop, the monitor of
 * the prefix consumed before it.  A state whose header does not go with `in`:
 * err[s] = FX_ERR_INVALID_ARG alone.  A rank word that points past the key's
 * rows is skipped.  May be called after any call; changes no state. */
int fx_kv_session_monitor(const fx_kv_batch* in, const uint32_t* rank, const fx_kv_out* out, const void* state,
                          void* hip_stream);
int fx_kv_session_monitor_host(const fx_kv_batch* in, const uint32_t* rank, const fx_kv_out* out, const void* state);

typedef struct fx_kv_monitor {
  const uint32_t* monitor; const uint32_t* mon_off;
  const uint32_t* rifl;    /* plane by arrival row: the word that names the command (the `dot` plane) */
  uint32_t num_streams, steps, keys;
} fx_kv_monitor;
/* check_monitors over pairs of streams.
 * pairs: [num_pairs * 2] = (stream of a, stream of b); a and b may be the same set.
 * diff:  [num_pairs * 2] = the smallest (key, position) at which the two per-key
 * sequences of rifl words differ (one ending before the other counts as a
 * difference at the shorter length), or (FX_KV_AGREE, FX_KV_AGREE).  A pair
 * that names a stream outside its set, or a stream whose mon_off row is not
 * ascending from 0 to at most steps or whose monitor rows in use hold an
 * arrival row >= steps (a stream fx_kv_execute left with an error), gets
 * (FX_KV_BAD_PAIR, FX_KV_BAD_PAIR) and nothing of it is read further.
 * Each side is held to its own num_streams and steps (a and b may be two
 * batches of different shapes).  mon_off[keys] == steps, a monitor that fills
 * every row, is legal; the rows in use are those below mon_off[keys], and what
 * the rows from there on hold is never read.
 * Refused with FX_ERR_INVALID_ARG: a null pointer (pairs and diff may be null
 * while num_pairs is 0), keys outside 1..FX_TABLE_MAX_KEYS, a.keys != b.keys. */
int fx_kv_monitor_compare(const fx_kv_monitor* a, const fx_kv_monitor* b, const uint32_t* pairs,
                          uint32_t num_pairs, uint32_t* diff, void* hip_stream);
int fx_kv_monitor_compare_host(const fx_kv_monitor* a, const fx_kv_monitor* b, const uint32_t* pairs,
                               uint32_t num_pairs, uint32_t* diff);
/* Op planes for generated streams: one op per row of stream s (global stream
 * stream_base + s), from one draw d of the counter RNG of fx_synth (C6) keyed
 * by (seed, global stream, row, purpose 16): with p = (d >> 32) % 100, a GET
 * if p < read_pct, a DELETE if p < read_pct + delete_pct, else a PUT of
 * 1 + d % (2^30 - 1).  Rows at or past lengths[s] (NULL: steps) and the pad
 * words of the plane are FX_KV_OP(FX_KV_EMPTY, 0): every word of
 * fx_plane_words(num_streams, steps) is written.  read_pct + delete_pct > 100
 * or stream_base + num_streams > 2^32: FX_ERR_INVALID_ARG.  The draw is keyed
 * by the row alone, so the call needs no key plane. */
int fx_kv_synth_ops(uint64_t seed, uint32_t stream_base, uint32_t read_pct, uint32_t delete_pct,
                    const uint32_t* lengths, uint32_t num_streams, uint32_t steps, uint32_t* ops, void* hip_stream);
int fx_kv_synth_ops_host(uint64_t seed, uint32_t stream_base, uint32_t read_pct, uint32_t delete_pct,
                         const uint32_t* lengths, uint32_t num_streams, uint32_t steps, uint32_t* ops);

/* --------------------------------- AggregatePending: command results per rifl */
/* What the reference does with the executors' results before a client sees
 * them (fantoch/src/executor/aggregate.rs:48-87, CommandResultBuilder,
 * command.rs:232-263): a command's partials, one per (rifl, key), are collected
 * and one CommandResult leaves when the last of them has arrived.  Here for a
 * batch, from the order plane any batched engine wrote.  Per stream, for k = 0
 * .. nexec - 1, with a = the arrival row of order row k (FX_ORDER_SCC_START
 * masked off), r = rifl[a] and c = count[a] & count_mask, or 0 when `process`
 * is not 0 and r >> 24 differs from it (wait_for is called by the process whose
 * client submitted the command, the dot's coordinator):
 *   c = 0   a result nobody waits for (aggregate.rs:58-62): head[a] =
 *           FX_PENDING_IGNORED, nothing else
 *   c = 1   a whole command: it is its own head, completes at once and never
 *           meets a builder (below)
 *   c > 1   no live builder for r: one is created with head row a, count c and
 *           got 0 (this stands in for the earlier wait_for).  A live builder
 *           for r: its count must equal c, else the stream stops with
 *           FX_ERR_INVALID_ARG.
 *   then, for c > 0: part[got][head] = a, head[a] = head, got += 1, and at got
 *           == count: index[head] = nready, ready[nready] = head, nready += 1
 *           and the builder is removed (aggregate.rs:66-78).  A later row of
 *           the same rifl starts a new command (the table executor's "starts a
 *           command of its own").
 * After the last row nopen = the builders still live.  A command is named by
 * its head row, the arrival row of its first executed partial; `part` is
 * FX_PENDING_MAX_PARTS planes indexed by head row, and the partials of a
 * command are listed in execution order (canonical C16; the reference keeps
 * them in a HashMap<Key, _>).
 * A stream that fails stops at that order row: nothing of that row or of later
 * rows is written, the rows before it stay valid, nready and nopen hold their
 * values at the stop.  A count above FX_PENDING_MAX_PARTS or an arrival row >=
 * steps: FX_ERR_INVALID_ARG; nexec > steps: FX_ERR_ORDER_OVERFLOW (nready =
 * nopen = 0).  Rows that are not executed, pad rows, pad streams and the
 * `ready` rows from nready on are not touched.
 * Not checked: add_partial's assert on a repeated key (command.rs:244-249; the
 * engines here already refuse a second event of a dot on one key), and a row of
 * count 1 against a live builder of its rifl (rifls are unique in the
 * reference; such a row never reads a table). */
#define FX_PENDING_MAX_PARTS FX_TABLE_MAX_CMD_KEYS
#define FX_PENDING_IGNORED 0xFFFFFFFFu
/* Tiers, as the table executor's.  ONCHIP: the live builders of a stream sit in
 * registers, FX_PENDING_ONCHIP_LIVE of them; the row that would create one more
 * stops the stream with FX_ERR_CAPACITY.  HBM: the builders sit in `state`
 * (fx_pending_state_bytes), buckets of 64 entries of 16 bytes, a builder of
 * rifl r in the first bucket from fx_pending_bucket(r, buckets) on (cyclic)
 * that had an entry never used; entries are not reused, and only a builder that
 * is live at the end of a 64-row chunk takes one, at most one per order row,
 * so the ceil(max(steps, 1) / 64) buckets never fill and no stream ends with
 * FX_ERR_CAPACITY.  The kernel clears the table itself. */
#define FX_PENDING_TIER_ONCHIP 0u
#define FX_PENDING_TIER_HBM 1u
#define FX_PENDING_ONCHIP_LIVE 64u
typedef struct fx_pending_batch {
  const uint32_t* order;   /* plane of an fx_order_batch                                        */
  const uint32_t* nexec;   /* [S] rows of `order` to take                                       */
  const uint32_t* rifl;    /* plane by arrival row (the `dot` plane of the table engines)       */
  const uint32_t* count;   /* plane by arrival row: the partials of the row's command           */
  uint32_t count_mask;     /* 0xFF lets a plane of FX_TABLE_PS_WORD be passed as it is; not 0   */
  uint32_t process;        /* 0, or the only source byte (rifl >> 24) whose rows are waited for */
  uint32_t num_streams, steps;
} fx_pending_batch;
typedef struct fx_pending_out {
  uint32_t* part;    /* FX_PENDING_MAX_PARTS planes by head row: plane j = the arrival row of
                        the command's j-th partial                                              */
  uint32_t* head;    /* plane by arrival row: the head row of its command, or FX_PENDING_IGNORED */
  uint32_t* ready;   /* plane: row i = the head row of the i-th completed command               */
  uint32_t* index;   /* plane by head row: the command's row in `ready`                         */
  uint32_t* nready;  /* [S] */
  uint32_t* nopen;   /* [S] */
  uint32_t* err;     /* [S] */
} fx_pending_out;
/* (mix(rifl) % buckets): mix(x) = x * 0x9E3779B1, then x ^= x >> 15 (32-bit); buckets >= 1. */
uint32_t fx_pending_bucket(uint32_t rifl, uint32_t buckets);
size_t fx_pending_state_bytes(uint32_t steps, uint32_t lanes);
/* One launch over num_lanes streams (stream_map NULL = the first num_lanes)
 * at one tier; state: NULL at ONCHIP, fx_pending_state_bytes(steps, num_lanes)
 * bytes at HBM (their content does not matter).  Refused with
 * FX_ERR_INVALID_ARG before any store: a null pointer, count_mask 0, a tier
 * that does not exist, state that does not go with the tier.  Device pointers;
 * asynchronous on hip_stream. */
int fx_pending_aggregate(const fx_pending_batch* in, const fx_pending_out* out, const uint32_t* stream_map,
                         uint32_t num_lanes, uint32_t tier, void* state, void* hip_stream);
/* Synchronous driver: every stream at ONCHIP, then the streams that stopped
 * with FX_ERR_CAPACITY whole at HBM; *reruns (optional) = streams rerun.
 * The return value is the call's own status (a refusal as fx_pending_aggregate,
 * FX_ERR_NO_DEVICE, FX_ERR_HIP); a stream's status is in out->err alone, so
 * FX_OK does not say that every stream ran to its end. */
int fx_pending_run(const fx_pending_batch* in, const fx_pending_out* out, void* hip_stream, uint32_t* reruns);
/* The same on the host (host pointers, identical bytes on both tiers, the
 * ONCHIP tier's capacity stop included).  No device needed. */
int fx_pending_aggregate_host(const fx_pending_batch* in, const fx_pending_out* out, uint32_t tier);
/* Resumable streams: the pending stage fed in pieces, behind an executor
 * session and beside fx_kv_advance.  A call takes order rows [done, nexec[s])
 * of every stream; done = where the stream's previous call stopped (0 with
 * FX_FLAG_INIT, which starts with no builders whatever `state` holds).  Rows
 * below done must not have changed and are not read again.  Between calls the
 * live builders sit in `state`: per stream a header {tag, steps, count_mask,
 * process, done, nready, live, err} and the HBM tier's table, cleared by
 * FX_FLAG_INIT only.  The outputs are fx_pending_aggregate's and cumulative.
 * After every call of a partition in which every nexec[s] <= steps does not
 * decrease, part, head, ready, index, nready, nopen and err equal in every
 * word what fx_pending_aggregate at FX_PENDING_TIER_HBM over this call's nexec
 * leaves on buffers of the same initial content; a stream that fails stops at
 * the same order row with the same status, and stays stopped: later calls
 * rewrite err[s] with that status and nothing else.
 *   a call with FX_FLAG_INIT writes nready, nopen and err whatever nexec[s] is
 *   nexec == done   err[s] is rewritten and nothing else
 *   nexec < done    err[s] = FX_ERR_INVALID_ARG for this call, state as it was
 *   nexec > steps   err[s] = FX_ERR_ORDER_OVERFLOW for this call, state as it
 *                   was (with FX_FLAG_INIT: nready = nopen = 0, no builders,
 *                   done = 0)
 * steps, count_mask and process are fixed for a session; a wrong tag or other
 * values than the header holds: err[s] = FX_ERR_INVALID_ARG and nothing else
 * of the stream read or written.  Refused with FX_ERR_INVALID_ARG before any
 * launch: a null pointer, count_mask 0, flags other than FX_FLAG_INIT.
 * state: fx_pending_session_bytes(steps, num_streams) bytes, indexed by
 * stream, opaque and per side (the host twin keeps its builders otherwise).
 * No stream ends with FX_ERR_CAPACITY: an entry of the table is taken at most
 * once per creating order row and never reused, so the ceil(max(steps, 1) /
 * 64) buckets of 64 entries never fill.  Asynchronous on hip_stream. */
size_t fx_pending_session_bytes(uint32_t steps, uint32_t num_streams);
int fx_pending_advance(const fx_pending_batch* in, const fx_pending_out* out, void* state, uint32_t flags,
                       void* hip_stream);
int fx_pending_advance_host(const fx_pending_batch* in, const fx_pending_out* out, void* state, uint32_t flags);

/* ------------------------------------------------- slot executor (FPaxos) */
/* SlotExecutor (fantoch_ps/src/executor/slot.rs:16-104): a stream is the
 * sequence of SlotExecutionInfo { slot, cmd } values one executor handles, in
 * arrival order.  Only the slot matters to the executor, so the input is one
 * plane of u32 slot numbers by arrival row.  Slots are 1-based (slot.rs:33-34);
 * the executor starts with next = 1 and nothing waiting.  Arrival row a with
 * slot s:
 *   s < next (which covers s == 0; slot.rs:55), or s already waiting
 *   (slot.rs:65-66): the stream stops at this row with FX_ERR_SLOT.
 *   Otherwise s waits, and while `next` waits (try_next_slot, slot.rs:89-96):
 *   it leaves the waiting set, order[nexec++] = its arrival row |
 *   FX_ORDER_SCC_START (every command its own group), release[that row] = a,
 *   next += 1.
 * A processed row whose command has not executed by the end of the stream has
 * release = FX_RELEASE_NONE.  FX_FLAG_EXECUTE_AT_COMMIT (slot.rs:57-58): every
 * row executes at its own step, order[a] = a | FX_ORDER_SCC_START, release[a] =
 * a; next never moves, so only s == 0 fails.
 * A slot above `steps` stops the stream with FX_ERR_CAPACITY on every tier and
 * on the host (not with FX_FLAG_EXECUTE_AT_COMMIT): a stream has at most
 * `steps` rows of distinct slots, so one of them above `steps` leaves a slot
 * below it that never arrives, a gap that cannot close within the stream; the
 * tables hold `steps` slots.  Nothing is written for the rows at or after a
 * failing row, the rows past a stream's length, or the order rows from nexec
 * on.  nexec and err per stream as in fx_order_batch.  Whole streams, from an
 * empty executor. */
typedef struct fx_slot_batch {
  const uint32_t* slot;     /* plane by arrival row: the slot of the row     */
  const uint32_t* lengths;  /* [S] rows per stream, or NULL = steps          */
  uint32_t num_streams;
  uint32_t steps;
} fx_slot_batch;
/* Tiers.  LANE: a lane per stream, the waiting slots next .. next +
 * FX_SLOT_LANE_WINDOW - 1 as a bitmap in registers and their arrival rows in
 * LDS; a row whose slot lies beyond that window stops the stream with
 * FX_ERR_CAPACITY.  At a row the checks go: FX_ERR_SLOT for s < next, then
 * the capacity, then FX_ERR_SLOT for a slot that waits.  SCAN: a wavefront per
 * stream, any reordering, over a table of `steps` words per stream in `state`
 * (fx_slot_state_bytes; the kernel clears it itself). */
#define FX_SLOT_TIER_LANE 0u
#define FX_SLOT_TIER_SCAN 1u
#define FX_SLOT_LANE_WINDOW 64u
size_t fx_slot_state_bytes(uint32_t steps, uint32_t lanes);
/* One launch over num_lanes streams (stream_map NULL = the first num_lanes) at
 * one tier; state: NULL at LANE, fx_slot_state_bytes(steps, num_lanes) bytes at
 * SCAN (their content does not matter).  Refused with FX_ERR_INVALID_ARG before
 * any store: a null pointer, a tier that does not exist, state that does not
 * go with the tier, steps >= 2^31, flags other than FX_FLAG_EXECUTE_AT_COMMIT.
 * Device pointers; asynchronous on hip_stream. */
int fx_slot_execute(const fx_slot_batch* in, const fx_order_batch* out, const uint32_t* stream_map,
                    uint32_t num_lanes, uint32_t tier, void* state, uint32_t flags, void* hip_stream);
/* Synchronous driver over the capacity-rerun chain.  With
 * FX_FLAG_FIRST_TIER(FX_SLOT_TIER_LANE) in flags: every stream at LANE, then
 * the streams that stopped with FX_ERR_CAPACITY whole at SCAN; *reruns
 * (optional) = streams rerun.  By default (no first tier, or SCAN) the chain is
 * SCAN alone and *reruns is 0: measured on 20,480 streams of 1,000 slots the
 * SCAN tier is three times faster than the LANE tier, which needs 64 streams
 * per wavefront and leaves most of the device idle at that batch size.  The
 * outputs are the same bytes either way.  The return value is the call's own
 * status, as fx_pending_run's (a first tier that does not exist:
 * FX_ERR_INVALID_ARG); a stream's status is in out->err alone. */
int fx_slot_run(const fx_slot_batch* in, const fx_order_batch* out, uint32_t flags, void* hip_stream,
                uint32_t* reruns);
/* The same on the host (host pointers): the bytes fx_slot_run leaves, which
 * are those of either tier for a stream that tier does not stop with
 * FX_ERR_CAPACITY.  No device needed. */
int fx_slot_execute_host(const fx_slot_batch* in, const fx_order_batch* out, uint32_t flags);
/* Resumable streams: the slot executor fed in pieces.  fx_slot_advance runs
 * rows [done, len) of every stream -- len = lengths[s] capped at steps, or
 * steps (lengths NULL); done = where the stream's previous call stopped (0
 * with FX_FLAG_INIT, which starts the stream from an empty executor whatever
 * `state` holds; the call clears its table itself).  The plane is the whole
 * stream's plane and arrival indices are plane rows.  Rows below done are not
 * read again; rows at or above len may hold anything.
 * The outputs are fx_slot_execute's and are cumulative: order row k is the
 * k-th executed command since row 0, nexec the running total.  After every
 * call, for any partition into calls, every word of order, release, nexec and
 * err equals what one fx_slot_execute at FX_SLOT_TIER_SCAN with this call's
 * lengths leaves on buffers of the same initial content, the words such a call
 * does not write included (rows at or after a failing row, order rows from
 * nexec on, rows past len, pad rows and pad streams).  A row that waits at the
 * end of a call has FX_RELEASE_NONE; a later call overwrites it with the
 * release step when its slot executes.
 *   len == done  nothing but the stream's state header is read; nexec[s] and
 *                err[s] are rewritten with their current values
 *   len < done   err[s] = FX_ERR_INVALID_ARG, nexec[s] keeps its value, state
 *                as it was: a later call with len >= done continues
 * steps and FX_FLAG_EXECUTE_AT_COMMIT are fixed for a session: the kernel
 * keeps them in the stream's state header beside a tag and validates the
 * header before it touches the table.  A wrong tag (a state that never saw
 * FX_FLAG_INIT), a call whose steps or commit flag differs, done > steps or
 * E (the executed count) > done: err[s] = FX_ERR_INVALID_ARG, state as it
 * was, nothing else of the stream written.  A stream that stopped with
 * FX_ERR_SLOT or FX_ERR_CAPACITY stays stopped: later calls handle nothing
 * for it and report the same err and nexec.  FX_ERR_CAPACITY (a slot above
 * steps, as on every tier) is final.  The statuses and their priority at a
 * row are fx_slot_execute's at SCAN.
 * Refused with FX_ERR_INVALID_ARG before any launch or store: a null in, out,
 * state or plane pointer, steps >= 2^31, flags other than FX_FLAG_INIT |
 * FX_FLAG_EXECUTE_AT_COMMIT.  After those checks no device gives
 * FX_ERR_NO_DEVICE; num_streams == 0 or steps == 0 returns FX_OK and does
 * nothing.
 * state: fx_slot_session_bytes(steps, num_streams) bytes, indexed by stream
 * (no stream_map); it belongs to the side (device or host) that initialised
 * it.  Asynchronous on hip_stream.  The LANE tier is not offered: it keeps its
 * waiting set in registers and LDS, and measured slower than SCAN at every
 * batch size tried. */
size_t fx_slot_session_bytes(uint32_t steps, uint32_t num_streams);
int fx_slot_advance(const fx_slot_batch* in, const fx_order_batch* out, void* state, uint32_t flags,
                    void* hip_stream);
/* The same on the host (host pointers, a state of its own): the same output
 * bytes for the same sequence of calls.  No device needed. */
int fx_slot_advance_host(const fx_slot_batch* in, const fx_order_batch* out, void* state, uint32_t flags);
/* Slot planes for generated streams: a leader that commits in slot order and
 * a network that reorders MChosen within bounds (fpaxos.rs:301-327).  Slot s
 * = 1 .. L of stream g (global stream stream_base + g, L = lengths[g] capped at
 * steps, NULL: steps) gets the key s + d % window, d the draw of the counter
 * RNG of fx_synth (C6) keyed by (seed, global stream, s, purpose 17); the
 * arrival order is the slots sorted by (key, s).  No slot is displaced by
 * `window` or more, so window <= FX_SLOT_LANE_WINDOW never leaves the LANE
 * tier.  Rows at or past L and the pad words of the plane are 0: every word of
 * fx_plane_words(num_streams, steps) is written.  window == 0, a null plane or
 * stream_base + num_streams > 2^32: FX_ERR_INVALID_ARG. */
int fx_slot_synth_generate(uint64_t seed, uint32_t stream_base, uint32_t num_streams, uint32_t steps,
                           const uint32_t* lengths, uint32_t window, uint32_t* slot_plane, void* hip_stream);
int fx_slot_synth_generate_host(uint64_t seed, uint32_t stream_base, uint32_t num_streams, uint32_t steps,
                                const uint32_t* lengths, uint32_t window, uint32_t* slot_plane);

/* ---------------------------------------------- single executor handle */
/* Config (fantoch/src/config.rs:5-45), the fields this path reads. */
typedef struct fx_config {
  uint32_t n;
  uint32_t f;
  uint32_t shard_count;                      /* must be 1 (partial replication out of scope) */
  uint32_t execute_at_commit;                /* config.rs execute_at_commit  */
  uint32_t executor_monitor_execution_order; /* config.rs: KVStore monitor (kvs.rs:29-39) */
} fx_config;

typedef struct fx_dot { uint32_t source; uint32_t seq; } fx_dot;       /* Dot  = Id<u8>  */
typedef struct fx_rifl { uint64_t source; uint64_t seq; } fx_rifl;     /* Rifl = Id<u64> */

/* ExecutorResult (fantoch/src/executor/mod.rs:169-174) with keys as u32 ids
 * (canonical C7) and payloads dropped. */
typedef struct fx_executor_result {
  fx_rifl rifl;
  uint32_t key;
  uint32_t read_only;
} fx_executor_result;

typedef struct fx_graph_executor fx_graph_executor;

/* Partial replication (Config::shard_count > 1, graph/mod.rs:82-406): the
 * streams run on the HBM wide tables with FX_FLAG_PARTIAL semantics.  A record
 * of kind FX_KIND_EXECUTED is RequestReply::Executed{dot}; RequestReply::Info
 * is an Add.  `req` holds per stream 1 + 2 req_cap words: word 0 = count, then
 * (step, parent dot) for every dep that went missing while no vertex waited on
 * it (the first PendingIndex::index of that dot, index.rs:180-198), the
 * candidates for out-requests (the caller keeps those its shard does not
 * replicate).  n = processes over all shards (<= 8); process ids 1..=n.
 * `state` = fx_partial_state_bytes(n, S) bytes; flags: FX_FLAG_INIT /
 * FX_FLAG_SAVE_STATE (resumable).  Device pointers, async on hip_stream. */
size_t fx_partial_state_bytes(uint32_t n, uint32_t num_streams);
int fx_batch_execute_partial(const fx_stream_batch* in, const fx_order_batch* out, void* state,
                             uint32_t step_begin, uint32_t step_end, uint32_t flags,
                             const uint32_t* init_frontier, uint32_t* req, uint32_t req_cap,
                             void* hip_stream);

/* Executor::new (executor.rs:34-51). NULL on bad config or no GPU.
 * The handle starts on tier 0 and, when its stream outgrows a tier, reruns its
 * log one tier up (0 -> 1 -> 2 -> 8): up to 16384 pending vertices, beyond
 * which the handle reports FX_ERR_CAPACITY (the reference's indexes are
 * unbounded, index.rs:18-51). */
fx_graph_executor* fx_graph_executor_new(uint8_t process_id, uint64_t shard_id, const fx_config* config);
/* Drop. */
void fx_graph_executor_free(fx_graph_executor* ex);
/* Executor::set_executor_index (executor.rs:53-56); only index 0 handles Adds. */
int fx_graph_executor_set_executor_index(fx_graph_executor* ex, uint32_t index);
/* Executor::handle(GraphExecutionInfo::Add{dot, cmd, deps}) (executor.rs:69-80).
 * keys: ids of the command's keys on this shard; deps in any order (the ABI
 * canonicalises to ascending, C1, and drops duplicates); now_ms = SysTime::millis(). */
int fx_graph_executor_handle_add(fx_graph_executor* ex, fx_dot dot, fx_rifl rifl,
                                 const uint32_t* keys, uint32_t nkeys, uint32_t read_only,
                                 const fx_dot* deps, uint32_t ndeps, uint64_t now_ms);
/* Partial replication (fx_config.shard_count > 1; n x shard_count <= 8 process
 * ids; the handle runs on the HBM wide tables, FX_FLAG_PARTIAL):
 * handle_add_sharded = handle(Add) and RequestReply::Info (mod.rs:390-393)
 * with each dep's Dependency::shards as a bitmask (deps/keys/mod.rs:19-22);
 * handle_executed = RequestReply::Executed for each dot (mod.rs:394-402);
 * requests drains DependencyGraph::requests (mod.rs:148-151) as (target
 * shard, dot) pairs, ascending; to_executors drains the dots added to the
 * executed clock (mod.rs:137-144, the Executed info of fetch_to_executors,
 * executor.rs:140-152), ascending.  Requests are served by a clone (below). */
int fx_graph_executor_handle_add_sharded(fx_graph_executor* ex, fx_dot dot, fx_rifl rifl,
                                         const uint32_t* keys, uint32_t nkeys, uint32_t read_only,
                                         const fx_dot* deps, const uint32_t* dep_shards, uint32_t ndeps,
                                         uint64_t now_ms, uint64_t cmd_shards);
/* cmd_shards: the shards the command has ops on (Command::replicated_by,
 * command.rs:90-92) as a bitmask; 0 = this handle's shard only.  An Info
 * reply's command is one this shard does not replicate, so its set (the
 * request_replies row's cmd_shards) is passed back as it is.  A Request for
 * a pending dot from a shard that replicates it is the reference's panic
 * (graph/mod.rs:308-316): FX_ERR_INVALID_ARG from handle_request / cleanup. */
int fx_graph_executor_handle_executed(fx_graph_executor* ex, const fx_dot* dots, uint32_t n, uint64_t now_ms);
int fx_graph_executor_requests(fx_graph_executor* ex, uint64_t* shards, fx_dot* dots, uint32_t cap,
                               uint32_t* n_out);
int fx_graph_executor_to_executors(fx_graph_executor* ex, fx_dot* dots, uint32_t cap, uint32_t* n_out);
/* Executor index > 0 of the same process (run mode clones the executor per
 * task and shares the VertexIndex, index.rs:21): a clone of a partial-
 * replication handle reads its main handle's vertices, keeps its own executed
 * clock (GraphExecutionInfo::Executed -> handle_executed_info, mod.rs:211-223),
 * serves Requests from other shards (handle_request / process_requests,
 * mod.rs:277-355: a vertex still pending -> RequestReply::Info with its deps,
 * an executed dot -> RequestReply::Executed, otherwise buffered) and retries
 * the buffered ones on cleanup (mod.rs:183-195).  Info replies carry the rifl
 * and deps; the command's ops stay with the caller (keyed by dot).  Free the
 * clone before its main handle.  Serving a request flushes the main handle. */
typedef struct fx_request_reply {
  uint64_t to_shard;
  uint32_t kind;      /* 1 = Info{dot, cmd, deps}, 0 = Executed{dot} */
  fx_dot dot;
  fx_rifl rifl;       /* Info: the command's rifl */
  uint32_t ndeps;     /* Info: deps at deps[first_dep, first_dep + ndeps) */
  uint32_t first_dep;
  uint64_t cmd_shards; /* Info: the command's shard set (cmd.shards(), as the reference ships the cmd) */
} fx_request_reply;
fx_graph_executor* fx_graph_executor_clone(fx_graph_executor* main);
int fx_graph_executor_handle_executed_info(fx_graph_executor* ex, const fx_dot* dots, uint32_t n);
int fx_graph_executor_handle_request(fx_graph_executor* ex, uint64_t from_shard, const fx_dot* dots, uint32_t n);
int fx_graph_executor_cleanup(fx_graph_executor* ex);
int fx_graph_executor_request_replies(fx_graph_executor* ex, fx_request_reply* out, uint32_t cap, fx_dot* deps,
                                      uint32_t* dep_shards, uint32_t deps_cap, uint32_t* n_out);
/* Test hook mirroring `queue.vertex_index.index(Vertex::new(..))` (mod.rs:1164-1306). */
int fx_graph_executor_index_only(fx_graph_executor* ex, fx_dot dot, fx_rifl rifl,
                                 const uint32_t* keys, uint32_t nkeys,
                                 const fx_dot* deps, uint32_t ndeps, uint64_t now_ms);
/* Test hook mirroring `queue.executed_clock = AEClock::from(..)` (mod.rs:1309-1315):
 * frontier[i] = highest contiguous executed seq of source i+1 (any u32). Only
 * before the first Add.  Sequences: fx_dot.seq is any u32; the device holds
 * seq - frontier (24 bits), so one handle spans 2^24 - 1 sequence numbers per
 * source above the frontier it starts from (FX_ERR_DOT_RANGE beyond). */
int fx_graph_executor_set_executed_frontier(fx_graph_executor* ex, const uint64_t* frontier, uint32_t n);
/* Executor::to_clients (executor.rs:95-97): pops up to cap results in execution order. */
int fx_graph_executor_to_clients(fx_graph_executor* ex, fx_executor_result* out, uint32_t cap, uint32_t* n_out);
/* Execution order as dots (DependencyGraph::commands_to_execute in the tests, mod.rs:158-160):
 * pops up to cap executed dots; scc_start[i] = 1 if out[i] opens a new SCC. */
int fx_graph_executor_drain_dots(fx_graph_executor* ex, fx_dot* out, uint8_t* scc_start, uint32_t cap, uint32_t* n_out);
/* Executor::metrics (executor.rs:107-109): histogram as (value, count) pairs
 * sorted by value; kind 0 = ExecutionDelay, 1 = ChainSize.  Returns pair count in *n_out. */
int fx_graph_executor_metrics(fx_graph_executor* ex, uint32_t kind, uint64_t* values,
                              uint64_t* counts, uint32_t cap, uint32_t* n_out);
/* Executor::monitor (executor.rs:111-113): the rifls executed on `key`, in order. */
int fx_graph_executor_monitor(fx_graph_executor* ex, uint32_t key, fx_rifl* out, uint32_t cap, uint32_t* n_out);
/* Pending vertices and the dot each waits on (0 source = none), ascending; debug/tests
 * (VertexIndex::monitor_pending, index.rs:53-103, reports the same information). */
int fx_graph_executor_pending(fx_graph_executor* ex, fx_dot* dots, fx_dot* waiting_on, uint32_t cap, uint32_t* n_out);
/* Executor::parallel (executor.rs:103-105). */
int fx_graph_executor_parallel(void);
/* Host<->device bytes this handle has moved so far (not in the reference; lets
 * a test check that draining after every Add moves bytes linear in the Adds). */
int fx_graph_executor_transfer_stats(const fx_graph_executor* ex, uint64_t* h2d, uint64_t* d2h);
/* Persistent-mode timing (diagnostics, tools/handle_latency): the first n of
 * FX_PERSIST_STATS counters, summed over the flushes: [0] flushes, [1] host wait
 * from doorbell to status (ns), [2] the kernel's compute, [3] its publish, [4]
 * polls, [5] poll round trips (100 MHz ticks), [6] the host's row preparation,
 * [7] order conversion (ns), [8] the compute in shader-clock cycles, [9] the
 * host's whole flush, [10] its reads after the wait, [11] its work before the
 * publish (ns), [12] executor iterations (DFS edges / frame pops, try and
 * check steps), [13] cycles in the Add's first step, [14] one-Add flushes
 * whose row the kernel took from the mailbox line (the rest read the ring). The
 * kernel's words are read only with FX_HANDLE_STATS=1 in the environment. */
#define FX_PERSIST_STATS 15
int fx_graph_executor_persist_stats(const fx_graph_executor* ex, uint64_t* out, uint32_t n);
/* Test hooks of the persistent mode (tests only; 0 = off), taking effect at
 * the kernel's next launch: skip_status_flush = k makes the k-th flush of a
 * launch publish no status, so the host's bounded wait expires; hold_ms keeps
 * the kernel resident, ignoring the stop request and its idle exit, until it
 * has been idle that long (at most 10 s: it still exits by itself), so the
 * host's stop request goes unanswered and the handle is abandoned. */
int fx_graph_executor_debug_hooks(fx_graph_executor* ex, uint32_t skip_status_flush, uint32_t hold_ms);

/* ------------------------------------------------------- quorum sizes */
#define FX_PROTOCOL_ATLAS 0u
#define FX_PROTOCOL_EPAXOS 1u
#define FX_PROTOCOL_BASIC 2u  /* fantoch/src/protocol/basic.rs (the simulator's own test protocol) */
/* Fast and write quorum sizes of the commit-stream producers:
 * Config::atlas_quorum_sizes (fantoch/src/config.rs:294-301) and
 * Config::epaxos_quorum_sizes (config.rs:303-312, f ignored).  The deps of a
 * commit are a union over the fast quorum (atlas.rs:404-475, epaxos.rs:370-428). */
int fx_quorum_sizes(uint32_t protocol, uint32_t n, uint32_t f, uint32_t* fast_quorum,
                    uint32_t* write_quorum);

/* --------------------------------------------------- batched simulator */
/* One simulated instance: Runner::new(planet, config, workload,
 * clients_per_process, process_regions, client_regions) + Runner::run
 * (fantoch/src/sim/runner.rs:64-231) with the GCP planet.  Regions are
 * indices into the planet's regions in name order (canonical C12); process i
 * (id i + 1) sits in process_regions[i]. */
#define FX_SIM_MAX_N 8u
#define FX_SIM_MAX_CLIENT_REGIONS 20u
typedef struct fx_sim_spec {
  uint64_t seed;                       /* canonical C6 RNG seed                       */
  uint64_t instance;                   /* global instance index (RNG stream)          */
  uint32_t protocol;                   /* FX_PROTOCOL_{ATLAS,EPAXOS,BASIC}            */
  uint32_t n, f;                       /* Config::new(n, f)                           */
  uint32_t gc_interval_ms;             /* Config::gc_interval (0 = None)              */
  uint32_t executed_notification_ms;   /* Config::executor_executed_notification_interval */
  uint32_t clients_per_region;         /* Runner::new clients_per_process             */
  uint32_t commands_per_client;        /* Workload::commands_per_client               */
  uint32_t keys_per_command;           /* Workload::keys_per_command (1 or 2)         */
  uint32_t conflict_rate;              /* KeyGen::ConflictPool::conflict_rate (%)     */
  uint32_t pool_size;                  /* KeyGen::ConflictPool::pool_size             */
  uint32_t read_only_pct;              /* Workload::read_only_percentage              */
  int32_t extra_sim_time_ms;           /* Runner::run(extra_sim_time): -1 = None      */
  uint32_t reorder_messages;           /* Runner::reorder_messages (C6 multiplier)    */
  uint32_t nfr;                        /* Config::nfr                                 */
  uint32_t num_client_regions;
  uint8_t process_regions[FX_SIM_MAX_N];
  uint8_t client_regions[FX_SIM_MAX_CLIENT_REGIONS];
} fx_sim_spec;

/* A batch of instances on one GPU (fx_sim_run): one wavefront per instance.
 * All instances of a batch share protocol family geometry: n, clients per
 * region, number of client regions, keys per command and pool size (the
 * conflict rate, f, seeds, regions and intervals may differ per instance).
 * The GPU path simulates Atlas and EPaxos (GraphExecutor protocols).  Two
 * kernels share the entry point: the all-on-chip one (sim_wave.hip: <= 32
 * clients per instance, no read-only commands, NFR or message reordering) and
 * the large-instance one (sim_big.hip: up to 65535 clients per instance,
 * read-only commands, NFR, message reordering; per-instance state in an HBM
 * arena of fx_sim_plan_large bytes, allocated stream-ordered by fx_sim_run).
 * fx_sim_run picks the first when the batch fits it, unless
 * FX_SIM_FLAG_LARGE is set. */
#define FX_SIM_FLAG_EXEC_NOTIFICATIONS 1u /* simulate the periodic executed notifications
                                             even when they cannot change the outcome
                                             (GraphExecutor::executed is None; they matter
                                             only for where a run with extra time stops) */
#define FX_SIM_FLAG_LARGE 2u              /* run the large-instance kernel */
#define FX_SIM_FLAG_GENERIC 4u            /* either kernel's build for run-time geometry even
                                             when the batch has one of the geometries compiled in
                                             (BASELINE configs[0]-[3]; same results, for A/B tests) */
#define FX_SIM_FLAG_ARENA_FILL 8u         /* tests: the large-instance kernel's arena starts filled
                                             with 0xA5 bytes instead of zeroed (the kernel must not
                                             read a word it did not write) */
typedef struct fx_sim_batch {
  const fx_sim_spec* specs;        /* [instances] device copy                          */
  const fx_sim_spec* host_specs;   /* [instances] host copy (validation, geometry)     */
  uint32_t instances;
  uint32_t flags;                  /* FX_SIM_FLAG_*                                     */
  const uint16_t* planet_ping;     /* device [planet_regions][planet_stride] ping (ms)  */
  const uint8_t* planet_rank;      /* device [planet_regions][planet_stride]: position of
                                      region b in region a's sorted order               */
  uint32_t planet_regions, planet_stride;
  uint32_t exec_cap;               /* executed dots kept per process (the rest counted) */
  uint32_t lat_cap;                /* latencies kept per client (0 = no latency log)    */
  uint32_t max_events;             /* per-instance event budget (0 = 2^32 - 1)          */
  uint32_t ring_entries;           /* messages in flight per instance, a pool shared by the
                                      process links (<= 65534; 0 = 16 n x clients per
                                      process region)                                   */
  uint32_t dot_slots;              /* live dots per instance, a pool shared by the
                                      coordinators (<= 256; 0 = min(64, 8 clients)); the
                                      large-instance kernel: <= 8 x 65536, direct-mapped
                                      per source (0 = 8 per client per process region) */
  uint32_t pad;
} fx_sim_batch;

/* per-instance counters (u64) */
#define FX_SIM_STAT_FAST 0u     /* [n] ProtocolMetricsKind::FastPath per process  */
#define FX_SIM_STAT_SLOW 8u     /* [n] SlowPath                                    */
#define FX_SIM_STAT_STABLE 16u  /* [n] Stable (commands garbage-collected; evaluated from the
                                   committed-frontier history at the end of the run) */
#define FX_SIM_STAT_EVENTS 24u  /* actions processed (executed notifications and GC traffic excluded) */
#define FX_SIM_STAT_END_MS 25u  /* simulation time when the run stopped            */
#define FX_SIM_STAT_TRACE 26u   /* hash of the processed action sequence, GC traffic excluded (debug) */
#define FX_SIM_STAT_SEQ 27u     /* schedule insertions                             */
#define FX_SIM_STAT_DEPS 28u    /* deps of every executor Add (sum over processes) */
#define FX_SIM_STAT_LAT_SUM 29u /* sum of every client command's latency (ms)       */
#define FX_SIM_STAT_ERR_SITE 30u /* where FX_ERR_SIM_CAPACITY was raised (source line) */
#define FX_SIM_STAT_FAST_READS 32u /* [n] FastPathReads (base.rs:229-243): read-only commands */
#define FX_SIM_STAT_SLOW_READS 40u /* [n] SlowPathReads                                   */
#define FX_SIM_STATS 48u

typedef struct fx_sim_output {  /* device buffers; NULL where not wanted */
  uint32_t* executed;           /* [instances][n][exec_cap] packed dots, execution order */
  uint32_t* executed_len;       /* [instances][n] commands executed per process     */
  uint32_t* latency_log;        /* [instances][clients][lat_cap] client latency (ms) */
  uint64_t* latency_hist;       /* [planet_regions][lat_bins] per client region, accumulated */
  uint64_t* chain_hist;         /* [chain_bins] ExecutorMetricsKind::ChainSize, accumulated */
  uint64_t* delay_hist;         /* [delay_bins] ExecutionDelay (ms), accumulated    */
  uint64_t* stats;              /* [instances][FX_SIM_STATS]                        */
  uint32_t* err;                /* [instances] FX_* status                           */
  uint32_t lat_bins, chain_bins, delay_bins, pad;
  uint32_t* dot_client;         /* [instances][n][exec_cap] client id (1-based) that submitted
                                   dot (p + 1, s) at [p][s - 1], or NULL (the rifl of an
                                   executed dot: the client's k-th dot is its command k + 1) */
} fx_sim_output;

/* LDS bytes one instance of `spec` needs at the given table sizes
 * (FX_ERR_UNSUPPORTED if it does not fit the GPU path). */
int fx_sim_plan(const fx_sim_spec* spec, uint32_t ring_entries, uint32_t dot_slots, uint32_t* lds_bytes);
/* Bytes of HBM arena one instance of `spec` takes in the large-instance kernel
 * at the given table sizes (0 = defaults); FX_ERR_UNSUPPORTED if it cannot run. */
int fx_sim_plan_large(const fx_sim_spec* spec, uint32_t ring_entries, uint32_t dot_slots, uint64_t* arena_bytes);
/* Runs every instance to completion (Runner::run, runner.rs:202-231); asynchronous. */
int fx_sim_run(const fx_sim_batch* batch, const fx_sim_output* out, void* hip_stream);
/* fx_sim_run, then (synchronously) reruns the instances that stopped with
 * FX_ERR_SIM_CAPACITY with larger tables (all-on-chip kernel: a 4x, at least
 * 256 n, message pool and 256 dot slots, then the large-instance kernel;
 * large-instance kernel: 2x the events and 4x the dots, twice), writing their
 * rows of every output in place.  Histograms stay exact: the samples the
 * failed runs added before failing are removed by replaying just those runs
 * at the first geometry (the kernel is deterministic per instance) and
 * subtracting.  An instance that fails at the larger geometry too keeps its
 * error and contributes no histogram samples.  *reruns (optional) = instances
 * rerun. */
int fx_sim_run_tiered(const fx_sim_batch* batch, const fx_sim_output* out, void* hip_stream, uint32_t* reruns);

/* Planet::from(dir) (fantoch/src/planet/mod.rs:38-54, dat.rs:20-94): regions
 * in name order; ping[a][b] (ms, `as u64` of the average) and rank[a][b] = the
 * position of b in a's (latency, name) order (Planet::sorted, mod.rs:122-140),
 * row stride `cap`.  With ping == NULL only *num_regions is filled.  names:
 * newline-separated region names (may be NULL). */
int fx_planet_load(const char* dir, uint32_t cap, uint32_t* num_regions, char* names, uint32_t names_bytes,
                   uint16_t* ping, uint8_t* rank);

/* ------------------------------------------------------- execution log */
/* Reader for the run mode's execution log: LengthDelimitedCodec frames
 * (4-byte big-endian length) of bincode-1 GraphExecutionInfo, as written by
 * execution_logger_task (fantoch/src/run/task/server/execution_logger.rs:11-55,
 * Rw::write fantoch/src/run/rw/mod.rs:66-77,93-100) and read back by
 * graph_executor_replay (fantoch_ps/src/bin/graph_executor_replay.rs:29-37,
 * Rw::recv rw/mod.rs:37-53).  Each Add becomes the arguments of
 * fx_graph_executor_handle_add: keys of `shard_id` interned to u32 ids in
 * first-seen order, deps as dots.  Request/RequestReply/Executed (partial
 * replication only) are parsed and counted in `others`, never executed. */
typedef struct fx_log_summary {
  uint64_t records;       /* frames                                          */
  uint64_t adds;          /* GraphExecutionInfo::Add frames                  */
  uint64_t others;        /* Request / RequestReply / Executed frames        */
  uint64_t keys;          /* sum of keys over the Adds (on shard_id)         */
  uint64_t deps;          /* sum of deps over the Adds                       */
  uint64_t distinct_keys; /* interned key ids                                */
} fx_log_summary;

typedef struct fx_log_add {
  fx_dot dot;
  fx_rifl rifl;
  uint64_t key_off;       /* into the keys array                             */
  uint64_t dep_off;       /* into the deps array                             */
  uint32_t nkeys;
  uint32_t ndeps;
  uint32_t read_only;     /* Command::read_only (command.rs:80-87)           */
  uint32_t pad;
} fx_log_add;

/* Validates the whole log and fills the summary (sizes for the decode call).
 * FX_ERR_LOG_FORMAT on a truncated frame, unknown tag, trailing bytes, or a
 * sequence above 2^32-1 (reference: Rw::recv's `expect`, rw/mod.rs:90). */
int fx_exec_log_scan(const uint8_t* buf, uint64_t len, uint64_t shard_id, fx_log_summary* out);
/* Decodes every Add in file order into caller-allocated arrays
 * (FX_ERR_CAPACITY if one is too small). */
int fx_exec_log_decode(const uint8_t* buf, uint64_t len, uint64_t shard_id, fx_log_add* adds,
                       uint64_t cap_adds, uint32_t* keys, uint64_t cap_keys, fx_dot* deps,
                       uint64_t cap_deps, fx_log_summary* out);

/* ------------------------------------------------- histogram statistics */
/* Histogram stats (histogram.rs:61-235) over (value, count) pairs sorted by value. */
typedef struct fx_hist_stats {
  double count, mean, stddev, cov, mdtm, min, max;
} fx_hist_stats;
int fx_hist_stats_compute(const uint64_t* values, const uint64_t* counts, uint32_t n, fx_hist_stats* out);
/* Histogram::percentile (histogram.rs:111-170). */
int fx_hist_percentile(const uint64_t* values, const uint64_t* counts, uint32_t n, double p, double* out);

/* ------------------------------------------------------------- runtime */
/* Number of visible GPUs; 0 means every compute entry point returns FX_ERR_NO_DEVICE. */
int fx_device_count(void);
/* Minimal device-memory plumbing for hosts without their own GPU runtime
 * bindings (a Rust/cgo/ctypes caller); torch callers may pass their own
 * device pointers and hipStream_t instead. */
int fx_dev_alloc(void** ptr, size_t bytes);
int fx_dev_free(void* ptr);
int fx_dev_memset(void* ptr, int value, size_t bytes, void* hip_stream);
int fx_dev_h2d(void* dst, const void* src, size_t bytes, void* hip_stream);
int fx_dev_d2h(void* dst, const void* src, size_t bytes, void* hip_stream);
int fx_dev_synchronize(void* hip_stream);
/* Elapsed milliseconds of the last fx_batch_execute launch on hip_stream,
 * measured with HIP events recorded on that stream around the kernel when
 * fx_profile_enable(1) is set (bench roofline; 0 disables the events). */
int fx_profile_enable(int on);
int fx_profile_last_exec_ms(float* ms);
/* Per-kernel duration of the last profiled launch: which = 0 the whole
 * executor launch (as fx_profile_last_exec_ms), 1 the group kernel and 2 the
 * lane kernel of FX_TIER_SPLIT (events recorded on each kernel's own stream);
 * FX_ERR_INVALID_ARG if that kernel did not run. */
int fx_profile_last_kernel_ms(uint32_t which, float* ms);
/* The last profiled launch of one kernel slot, timed by HIP events on the
 * stream it ran on: slot = an executor tier (FX_TIER_*, fx_batch_execute and
 * the tiered drivers' launches), FX_PROFILE_SLOT_PRED + FX_PRED_TIER_* (the
 * predecessors executor), FX_PROFILE_SLOT_TABLE + FX_TABLE_TIER_* (the table
 * executor; + 2: fx_table_advance); FX_ERR_INVALID_ARG if it did not run since fx_profile_enable(1). */
#define FX_PROFILE_SLOT_PRED 16u
#define FX_PROFILE_SLOT_TABLE 20u
#define FX_PROFILE_SLOTS 24u
int fx_profile_slot_ms(uint32_t slot, float* ms);
const char* fx_status_string(int status);
const char* fx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FANTOCH_AMD_H */
