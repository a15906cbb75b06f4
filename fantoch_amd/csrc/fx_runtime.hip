// fx_runtime.hip — the library's runtime plumbing: device count, version and
// status strings, the fx_dev_* memory calls, and the HIP-event profile state
// behind the fx_profile_* entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fantoch_amd.h"
#include "fx_internal.h"

namespace fx {

static bool g_profile = false;
static hipEvent_t g_ev0 = nullptr, g_ev1 = nullptr;
static bool g_ev_valid = false;
// split-tier kernels: [1] group kernel (caller's stream), [2] lane kernel (aux stream)
static hipEvent_t g_kev[3][2] = {};
static bool g_kev_valid[3] = {};

// per-slot kernel events (fx_profile_slot_ms): slot = executor tier
// (fx_batch_execute), FX_PROFILE_SLOT_PRED + tier (fx_pred_execute); each
// holds its slot's last launch
static hipEvent_t g_sev[FX_PROFILE_SLOTS][2] = {};
static bool g_sev_valid[FX_PROFILE_SLOTS] = {};
void profile_slot_record(uint32_t slot, bool end, hipStream_t s) {
  if (!g_profile || slot >= FX_PROFILE_SLOTS) return;
  hipEvent_t& e = g_sev[slot][end ? 1 : 0];
  if (!e && hipEventCreate(&e) != hipSuccess) return;
  (void)hipEventRecord(e, s);
  g_sev_valid[slot] = end;
}

void split_profile_record(int which, bool end, hipStream_t s) {
  if (!g_profile || which < 1 || which > 2) return;
  hipEvent_t& e = g_kev[which][end ? 1 : 0];
  if (!e && hipEventCreate(&e) != hipSuccess) return;
  (void)hipEventRecord(e, s);
  g_kev_valid[which] = end;
}

int profile_exec_begin(hipStream_t hs) {
  if (!g_profile) return FX_OK;
  if (!g_ev0 && (hipEventCreate(&g_ev0) != hipSuccess || hipEventCreate(&g_ev1) != hipSuccess)) return FX_ERR_HIP;
  (void)hipEventRecord(g_ev0, hs);
  g_kev_valid[1] = g_kev_valid[2] = false;
  return FX_OK;
}

void profile_exec_end(bool ok, hipStream_t hs) {
  if (!g_profile) return;
  (void)hipEventRecord(g_ev1, hs);
  g_ev_valid = ok;
}

}  // namespace fx

using namespace fx;

extern "C" {

int fx_device_count(void) {
  static int count = -1;
  if (count < 0) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    count = c;
  }
  return count;
}

const char* fx_version(void) { return "fantoch_amd 0.1.0 (gfx950)"; }

const char* fx_status_string(int s) {
  switch (s) {
    case FX_OK: return "ok";
    case FX_ERR_INVALID_ARG: return "invalid argument";
    case FX_ERR_CAPACITY: return "tier capacity exceeded";
    case FX_ERR_DOUBLE_INDEX: return "tried to index already indexed dot";
    case FX_ERR_DEPS_UNSORTED: return "deps not strictly ascending";
    case FX_ERR_DOT_RANGE: return "dot out of range";
    case FX_ERR_HIP: return "HIP runtime error";
    case FX_ERR_UNSUPPORTED: return "unsupported (partial replication)";
    case FX_ERR_ORDER_OVERFLOW: return "order plane overflow";
    case FX_ERR_TIME_RANGE: return "time out of range";
    case FX_ERR_NO_DEVICE: return "no GPU device";
    case FX_ERR_LOG_FORMAT: return "malformed execution log";
    case FX_ERR_SIM_CAPACITY: return "simulated instance outgrew its launch geometry";
    case FX_ERR_SIM_LATE: return "simulated message found no state for its dot";
    case FX_ERR_SIM_EVENTS: return "simulated instance exceeded its event budget";
    case FX_ERR_TIMEOUT: return "a drop-in handle's wait for its resident kernel passed the deadline";
    case FX_ERR_VOTE_RANGE: return "vote range invalid or without a new vote";
    case FX_ERR_SLOT: return "slot 0, already executed or already waiting";
    default: return "unknown";
  }
}

int fx_profile_enable(int on) {
  g_profile = on != 0;
  g_ev_valid = false;
  g_kev_valid[1] = g_kev_valid[2] = false;
  for (uint32_t i = 0; i < FX_PROFILE_SLOTS; ++i) g_sev_valid[i] = false;
  return FX_OK;
}

int fx_profile_slot_ms(uint32_t slot, float* ms) {
  if (!ms || slot >= FX_PROFILE_SLOTS) return FX_ERR_INVALID_ARG;
  if (!g_sev_valid[slot]) return FX_ERR_INVALID_ARG;
  if (hipEventSynchronize(g_sev[slot][1]) != hipSuccess) return FX_ERR_HIP;
  return hipEventElapsedTime(ms, g_sev[slot][0], g_sev[slot][1]) == hipSuccess ? FX_OK : FX_ERR_HIP;
}

int fx_profile_last_kernel_ms(uint32_t which, float* ms) {
  if (!ms) return FX_ERR_INVALID_ARG;
  if (which == 0) return fx_profile_last_exec_ms(ms);
  if (which > 2 || !g_kev_valid[which]) return FX_ERR_INVALID_ARG;
  if (hipEventSynchronize(g_kev[which][1]) != hipSuccess) return FX_ERR_HIP;
  return hipEventElapsedTime(ms, g_kev[which][0], g_kev[which][1]) == hipSuccess ? FX_OK : FX_ERR_HIP;
}

int fx_profile_last_exec_ms(float* ms) {
  if (!ms || !g_ev_valid) return FX_ERR_INVALID_ARG;
  if (hipEventSynchronize(g_ev1) != hipSuccess) return FX_ERR_HIP;
  return hipEventElapsedTime(ms, g_ev0, g_ev1) == hipSuccess ? FX_OK : FX_ERR_HIP;
}

int fx_dev_alloc(void** ptr, size_t bytes) {
  if (!ptr) return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  return hipMalloc(ptr, bytes ? bytes : 16) == hipSuccess ? FX_OK : FX_ERR_HIP;
}
int fx_dev_free(void* ptr) { return hipFree(ptr) == hipSuccess ? FX_OK : FX_ERR_HIP; }
int fx_dev_memset(void* ptr, int value, size_t bytes, void* hs) {
  return hipMemsetAsync(ptr, value, bytes, (hipStream_t)hs) == hipSuccess ? FX_OK : FX_ERR_HIP;
}
int fx_dev_h2d(void* dst, const void* src, size_t bytes, void* hs) {
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)hs) == hipSuccess ? FX_OK : FX_ERR_HIP;
}
int fx_dev_d2h(void* dst, const void* src, size_t bytes, void* hs) {
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)hs) == hipSuccess ? FX_OK : FX_ERR_HIP;
}
int fx_dev_synchronize(void* hs) {
  return hipStreamSynchronize((hipStream_t)hs) == hipSuccess ? FX_OK : FX_ERR_HIP;
}

}  // extern "C"
