// fantoch_amd.hpp — C++ host mirror of the reference's executor surface over
// the C-ABI (fantoch_amd.h).  Names, argument meaning and error behaviour
// follow the Rust items (a panic there is an exception here):
//   Dot / Rifl ............. fantoch/src/id.rs:7-27
//   Config ................. fantoch/src/config.rs:5-102 (fields this path reads)
//   Command ................ fantoch/src/command.rs:12-72 (keys as u32 ids, C7)
//   Dependency ............. fantoch_ps/src/protocol/common/graph/deps/keys/mod.rs:18-35
//   GraphExecutionInfo::add  fantoch_ps/src/executor/graph/executor.rs:197-218
//   ExecutorResult ......... fantoch/src/executor/mod.rs:169-184
//   GraphExecutor .......... fantoch_ps/src/executor/graph/executor.rs:19-114
//                            (the `Executor` trait, fantoch/src/executor/mod.rs:27-89)
//   read_execution_log ..... Rw::recv over an execution log (fantoch/src/run/rw/mod.rs:37-53,
//                            written by run/task/server/execution_logger.rs:11-55)
//   replay_execution_log ... fantoch_ps/src/bin/graph_executor_replay.rs:13-38
#pragma once
#include <cstdint>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "fantoch_amd.h"

namespace fantoch_amd {

using ProcessId = uint8_t;
using ShardId = uint64_t;
using Key = uint32_t;

struct Dot {
  ProcessId source = 0;
  uint64_t sequence = 0;
  Dot() = default;
  Dot(ProcessId s, uint64_t q) : source(s), sequence(q) {}
  bool operator<(const Dot& o) const {
    return source != o.source ? source < o.source : sequence < o.sequence;
  }
  bool operator==(const Dot& o) const { return source == o.source && sequence == o.sequence; }
};

struct Rifl {
  uint64_t source = 0;
  uint64_t sequence = 0;
  Rifl() = default;
  Rifl(uint64_t s, uint64_t q) : source(s), sequence(q) {}
  bool operator==(const Rifl& o) const { return source == o.source && sequence == o.sequence; }
  bool operator<(const Rifl& o) const {
    return source != o.source ? source < o.source : sequence < o.sequence;
  }
};

struct Config {
  uint32_t n = 0, f = 0, shard_count = 1;
  bool execute_at_commit = false;
  bool executor_monitor_execution_order = false;
  Config(uint32_t n_, uint32_t f_) : n(n_), f(f_) {}  // Config::new (config.rs:52-102)
};

struct Command {
  Rifl rifl;
  std::vector<Key> keys;
  bool read_only = false;
  // Command::from(rifl, [(key, op)]) with the payloads dropped (C7)
  static Command from(Rifl r, std::vector<Key> ks, bool read_only = false) {
    Command c;
    c.rifl = r;
    c.keys = std::move(ks);
    c.read_only = read_only;
    return c;
  }
};

struct Dependency {
  Dot dot;
};

struct GraphExecutionInfo {
  Dot dot;
  Command cmd;
  std::vector<Dependency> deps;
  static GraphExecutionInfo add(Dot d, Command c, std::vector<Dependency> deps) {
    return GraphExecutionInfo{d, std::move(c), std::move(deps)};
  }
};

struct ExecutorResult {
  Rifl rifl;
  Key key;
};

enum class ExecutorMetricsKind : uint32_t { ExecutionDelay = 0, ChainSize = 1 };

class Error : public std::runtime_error {
 public:
  int status;
  explicit Error(int s) : std::runtime_error(fx_status_string(s)), status(s) {}
};

inline void check(int s) {
  if (s != FX_OK) throw Error(s);
}

class GraphExecutor {
 public:
  // Executor::new (executor.rs:34-51)
  GraphExecutor(ProcessId process_id, ShardId shard_id, const Config& config) {
    fx_config c{config.n, config.f, config.shard_count, config.execute_at_commit ? 1u : 0u,
                config.executor_monitor_execution_order ? 1u : 0u};
    h_ = fx_graph_executor_new(process_id, shard_id, &c);
    if (!h_) throw Error(fx_device_count() <= 0 ? FX_ERR_NO_DEVICE : FX_ERR_INVALID_ARG);
  }
  GraphExecutor(const GraphExecutor&) = delete;
  GraphExecutor& operator=(const GraphExecutor&) = delete;
  ~GraphExecutor() { fx_graph_executor_free(h_); }

  void set_executor_index(uint32_t index) { check(fx_graph_executor_set_executor_index(h_, index)); }

  // Executor::handle (executor.rs:69-93); only Add exists with shard_count == 1
  void handle(const GraphExecutionInfo& info, uint64_t time_ms) {
    std::vector<fx_dot> deps;
    for (const auto& d : info.deps) deps.push_back(fx_dot{d.dot.source, (uint32_t)d.dot.sequence});
    check(fx_graph_executor_handle_add(h_, fx_dot{info.dot.source, (uint32_t)info.dot.sequence},
                                       fx_rifl{info.cmd.rifl.source, info.cmd.rifl.sequence},
                                       info.cmd.keys.data(), (uint32_t)info.cmd.keys.size(),
                                       info.cmd.read_only ? 1u : 0u, deps.data(),
                                       (uint32_t)deps.size(), time_ms));
  }

  // Executor::to_clients (executor.rs:95-97)
  std::optional<ExecutorResult> to_clients() {
    fx_executor_result r;
    uint32_t got = 0;
    check(fx_graph_executor_to_clients(h_, &r, 1, &got));
    if (!got) return std::nullopt;
    return ExecutorResult{Rifl(r.rifl.source, r.rifl.seq), r.key};
  }

  // Executor::to_clients_iter (mod.rs:58-60)
  std::vector<ExecutorResult> to_clients_iter() {
    std::vector<ExecutorResult> v;
    while (auto r = to_clients()) v.push_back(*r);
    return v;
  }

  // DependencyGraph::commands_to_execute as dots (mod.rs:158-160)
  std::vector<std::pair<Dot, bool>> drain_dots() {
    std::vector<std::pair<Dot, bool>> v;
    fx_dot buf[256];
    uint8_t start[256];
    while (true) {
      uint32_t got = 0;
      check(fx_graph_executor_drain_dots(h_, buf, start, 256, &got));
      for (uint32_t i = 0; i < got; ++i) v.emplace_back(Dot((ProcessId)buf[i].source, buf[i].seq), start[i] != 0);
      if (got < 256) break;
    }
    return v;
  }

  static bool parallel() { return fx_graph_executor_parallel() != 0; }

  // Executor::metrics (executor.rs:107-109): collected histogram of a kind
  std::map<uint64_t, uint64_t> metrics(ExecutorMetricsKind kind) {
    uint32_t n = 0;
    check(fx_graph_executor_metrics(h_, (uint32_t)kind, nullptr, nullptr, 0, &n));
    std::vector<uint64_t> v(n), c(n);
    check(fx_graph_executor_metrics(h_, (uint32_t)kind, v.data(), c.data(), n, &n));
    std::map<uint64_t, uint64_t> m;
    for (uint32_t i = 0; i < n; ++i) m[v[i]] = c[i];
    return m;
  }

  // Executor::monitor -> ExecutionOrderMonitor::get_order(key) (monitor.rs:44-46)
  std::vector<Rifl> monitor_order(Key key) {
    uint32_t n = 0;
    check(fx_graph_executor_monitor(h_, key, nullptr, 0, &n));
    std::vector<fx_rifl> r(n);
    check(fx_graph_executor_monitor(h_, key, r.data(), n, &n));
    std::vector<Rifl> out;
    for (const auto& x : r) out.emplace_back(x.source, x.seq);
    return out;
  }

  fx_graph_executor* raw() { return h_; }

 private:
  fx_graph_executor* h_ = nullptr;
};

// Decodes every GraphExecutionInfo::Add of an execution log (LengthDelimitedCodec
// frames of bincode-1) into GraphExecutionInfo values, keys of `shard_id` interned
// in first-seen order.  A malformed log throws Error(FX_ERR_LOG_FORMAT), as
// Rw::recv's `expect` panics (rw/mod.rs:90).  `others` counts the
// Request / RequestReply / Executed frames (partial replication only).
inline std::vector<GraphExecutionInfo> read_execution_log(const std::vector<uint8_t>& bytes,
                                                          ShardId shard_id = 0,
                                                          uint64_t* others = nullptr) {
  fx_log_summary sum{};
  check(fx_exec_log_scan(bytes.data(), bytes.size(), shard_id, &sum));
  std::vector<fx_log_add> adds(sum.adds);
  std::vector<uint32_t> keys(sum.keys);
  std::vector<fx_dot> deps(sum.deps);
  check(fx_exec_log_decode(bytes.data(), bytes.size(), shard_id, adds.data(), sum.adds, keys.data(),
                           sum.keys, deps.data(), sum.deps, &sum));
  if (others) *others = sum.others;
  std::vector<GraphExecutionInfo> out;
  out.reserve(adds.size());
  for (const auto& a : adds) {
    std::vector<Key> ks(keys.begin() + a.key_off, keys.begin() + a.key_off + a.nkeys);
    std::vector<Dependency> ds;
    for (uint32_t i = 0; i < a.ndeps; ++i) {
      const fx_dot& d = deps[a.dep_off + i];
      ds.push_back(Dependency{Dot((ProcessId)d.source, d.seq)});
    }
    out.push_back(GraphExecutionInfo::add(
        Dot((ProcessId)a.dot.source, a.dot.seq),
        Command::from(Rifl(a.rifl.source, a.rifl.seq), std::move(ks), a.read_only != 0), std::move(ds)));
  }
  return out;
}

// graph_executor_replay: process 1, shard 0, Config::new(n, f); every Add in file
// order into `executor` at time `time_ms`.
inline void replay_execution_log(GraphExecutor& executor, const std::vector<uint8_t>& bytes,
                                 uint64_t time_ms = 0) {
  uint64_t others = 0;
  auto infos = read_execution_log(bytes, 0, &others);
  if (others) throw Error(FX_ERR_UNSUPPORTED);
  for (const auto& info : infos) executor.handle(info, time_ms);
}

// AggregatePending for a batch (fx_pending_run: every stream on the ONCHIP
// tier, the ones that run out of builders again on the HBM tier).  Device
// pointers; a stream's status lands in out.err alone, a call that is refused
// or cannot run throws.  Returns the streams that ran again.
inline uint32_t aggregate_pending(const fx_pending_batch& in, const fx_pending_out& out, void* hip_stream = nullptr) {
  uint32_t reruns = 0;
  check(fx_pending_run(&in, &out, hip_stream, &reruns));
  return reruns;
}
// The same on the host (identical bytes; tier: FX_PENDING_TIER_*).
inline void aggregate_pending_host(const fx_pending_batch& in, const fx_pending_out& out,
                                   uint32_t tier = FX_PENDING_TIER_HBM) {
  check(fx_pending_aggregate_host(&in, &out, tier));
}
// AggregatePending fed in pieces behind an executor session (fx_pending_advance):
// order rows [done, nexec) of every stream, the live builders kept in `state`
// (aggregate_pending_session_bytes; `start` begins the session with none).  The
// outputs are cumulative: the `ready` rows between the nready before a call and
// the nready after it are the commands that call completed.
inline size_t aggregate_pending_session_bytes(uint32_t steps, uint32_t num_streams) {
  return fx_pending_session_bytes(steps, num_streams);
}
inline void aggregate_pending_advance(const fx_pending_batch& in, const fx_pending_out& out, void* state, bool start,
                                      void* hip_stream = nullptr) {
  check(fx_pending_advance(&in, &out, state, start ? FX_FLAG_INIT : 0u, hip_stream));
}
// The same on the host (identical output bytes, a state of its own).
inline void aggregate_pending_advance_host(const fx_pending_batch& in, const fx_pending_out& out, void* state,
                                           bool start) {
  check(fx_pending_advance_host(&in, &out, state, start ? FX_FLAG_INIT : 0u));
}

// Caesar-shaped commit streams for the predecessors executor (fx_pred_synth_*:
// the model is fx_pred_synth.h's).  The shape of a parameter set; a refused
// set throws.
struct PredSynthShape {
  uint32_t num_streams = 0, steps = 0, dmax = 0;
};
inline PredSynthShape pred_synth_shape(const fx_pred_synth_params& p) {
  PredSynthShape s;
  check(fx_pred_synth_shape(&p, &s.num_streams, &s.steps, &s.dmax));
  return s;
}
// Device planes (asynchronous on hip_stream), and the same bytes on the host.
inline void pred_synth_generate(const fx_pred_synth_params& p, const fx_pred_synth_planes& planes,
                                void* hip_stream = nullptr) {
  check(fx_pred_synth_generate(&p, &planes, hip_stream));
}
inline void pred_synth_generate_host(const fx_pred_synth_params& p, const fx_pred_synth_planes& planes) {
  check(fx_pred_synth_generate_host(&p, &planes));
}

// SlotExecutor (fantoch_ps/src/executor/slot.rs:16-104) for a batch: a stream is
// the slots of the SlotExecutionInfo values one executor handles, in arrival
// order (SlotExecutionInfo::new(slot, cmd), slot.rs:112-116; the command of a
// row is the caller's, named by the arrival row in the outputs).  Device
// pointers; a stream's status (FX_ERR_SLOT where the reference's asserts fail)
// lands in out.err alone, a call that is refused or cannot run throws.
class SlotExecutor {
 public:
  // Executor::new (slot.rs:31-48); Config::execute_at_commit is the one field read
  explicit SlotExecutor(const Config& config) : flags_(config.execute_at_commit ? FX_FLAG_EXECUTE_AT_COMMIT : 0u) {}

  // Executor::handle over every row of every stream (slot.rs:50-69): every
  // stream on the SCAN tier, or with lane_first on the LANE tier and the ones
  // reordered beyond its window again on the SCAN tier.  Returns the streams
  // that ran again.
  uint32_t handle(const fx_slot_batch& in, const fx_order_batch& out, void* hip_stream = nullptr,
                  bool lane_first = false) const {
    uint32_t reruns = 0;
    check(fx_slot_run(&in, &out, flags_ | (lane_first ? FX_FLAG_FIRST_TIER(FX_SLOT_TIER_LANE) : 0u), hip_stream, &reruns));
    return reruns;
  }
  // The same on the host (identical bytes).
  void handle_host(const fx_slot_batch& in, const fx_order_batch& out) const {
    check(fx_slot_execute_host(&in, &out, flags_));
  }

  static bool parallel() { return false; }  // slot.rs:75-77

 private:
  uint32_t flags_;
};

}  // namespace fantoch_amd
