// table_synth.hip — synthetic Tempo vote streams generated on the device
// (fx_table_synth_lengths / fx_table_synth_generate; the model: fx_table_synth.h).
//
// A stream is sequential (every command reads the clocks the last one left),
// so the parallelism is across streams: one lane per stream, one wavefront per
// 64-stream plane tile, and a wavefront's stores of one step row land in one
// 1 KiB tile.  Two launches of the same walk: k_table_synth<.., false> counts
// the events of every delivery slot into scratch[slot][stream] (slot-major: a
// wavefront's lanes touch adjacent words) and turns the counts into first rows;
// k_table_synth<.., true> walks the same draws and stores every event at its
// slot's cursor.  Per-stream state (clocks[key][process], the coordinators'
// command counts) is word w of lane l at LDS word 64 w + l -- the lanes of an
// access hit 64 consecutive banks -- while (keys + 1) n <=
// FX_TABLE_SYNTH_ONCHIP_WORDS, else at scratch[w][stream].  No lane reads
// another lane's words: no barrier, no cross-lane operation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "fx_table_synth.h"

namespace {

struct SynthArgs {
  fx_table_synth_params p;
  uint32_t* slots;    // [ts_slots][spad]
  uint32_t* state;    // [ts_state_words][spad], off-chip state only
  uint32_t* lengths;  // [S]
  uint32_t spad, nslots;
  fx::TsOut out;      // EMIT only (stream filled in per lane)
};

template <bool LDS, bool EMIT>
__global__ __launch_bounds__(64) void k_table_synth(const SynthArgs a) {
  extern __shared__ uint32_t lds_state[];
  const uint32_t s = blockIdx.x * 64u + threadIdx.x;
  if (s >= a.p.streams) return;  // pad lanes of the last tile: their rows stay zero
  const fx::TsStream ts = fx::ts_stream(a.p, s);
  const fx::TsWords slots{a.slots + s, a.spad};
  fx::TsOut out = a.out;
  out.stream = s;
  if (LDS)
    fx::ts_walk<EMIT>(ts, fx::TsWords{lds_state + threadIdx.x, 64}, slots, out);
  else
    fx::ts_walk<EMIT>(ts, fx::TsWords{a.state + s, a.spad}, slots, out);
  if (!EMIT) a.lengths[s] = fx::ts_prefix(slots, a.nslots);
}

// the state on chip while it fits, else in scratch
template <bool EMIT>
bool launch(const SynthArgs& a, hipStream_t hs) {
  const uint32_t words = fx::ts_state_words(a.p);
  const dim3 grid(a.spad / 64u);
  if (words <= FX_TABLE_SYNTH_ONCHIP_WORDS)
    hipLaunchKernelGGL((k_table_synth<true, EMIT>), grid, dim3(64), (size_t)words * 256u, hs, a);
  else
    hipLaunchKernelGGL((k_table_synth<false, EMIT>), grid, dim3(64), 0, hs, a);
  return hipGetLastError() == hipSuccess;
}

// Both passes share the arguments; the counting pass is waited for and the
// longest stream returned.
int count_pass(const fx_table_synth_params* p, uint32_t* lengths_dev, void* scratch, hipStream_t hs, SynthArgs& a,
               uint32_t* max_len) {
  a.p = *p;
  a.spad = (p->streams + 63u) / 64u * 64u;
  a.nslots = fx::ts_slots(*p);
  a.slots = (uint32_t*)scratch;
  a.state = a.slots + (size_t)a.nslots * a.spad;
  a.lengths = lengths_dev;
  a.out = fx::TsOut{};
  const uint32_t S = p->streams;
  if (max_len) *max_len = 0;
  if (S == 0) return FX_OK;
  if (hipMemsetAsync(a.slots, 0, (size_t)a.nslots * a.spad * 4, hs) != hipSuccess) return FX_ERR_HIP;
  if (!launch<false>(a, hs)) return FX_ERR_HIP;
  std::vector<uint32_t> len(S);
  if (hipMemcpyAsync(len.data(), lengths_dev, (size_t)S * 4, hipMemcpyDeviceToHost, hs) != hipSuccess ||
      hipStreamSynchronize(hs) != hipSuccess)
    return FX_ERR_HIP;
  if (max_len) *max_len = *std::max_element(len.begin(), len.end());
  return FX_OK;
}

}  // namespace

extern "C" int fx_table_synth_lengths(const fx_table_synth_params* p, uint32_t* lengths_dev, void* scratch,
                                      void* hip_stream, uint32_t* max_len) {
  const int st = fx::ts_check(p);
  if (st) return st;
  if (!lengths_dev || !scratch) return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  SynthArgs a;
  return count_pass(p, lengths_dev, scratch, (hipStream_t)hip_stream, a, max_len);
}

extern "C" int fx_table_synth_generate(const fx_table_synth_params* p, const fx_table_synth_planes* o, uint32_t steps,
                                       void* scratch, void* hip_stream) {
  int st = fx::ts_check(p);
  if (st) return st;
  if (!o || !o->hdr || !o->dot || !o->clock || !o->votes || !o->lengths || (!o->nkeys && p->kmax > 1) || !scratch)
    return FX_ERR_INVALID_ARG;
  if (fx_device_count() <= 0) return FX_ERR_NO_DEVICE;
  hipStream_t hs = (hipStream_t)hip_stream;
  SynthArgs a;
  uint32_t longest = 0;
  st = count_pass(p, o->lengths, scratch, hs, a, &longest);
  if (st) return st;
  if (longest > steps) return FX_ERR_CAPACITY;  // (the lengths are written, no plane is)
  // rows no stream reaches and the pad streams of the last tile: zero
  a.out = fx::TsOut{o->hdr, o->dot, o->clock, o->votes, o->nkeys, fx_plane_words(p->streams, steps), steps, 0};
  if (a.out.plane == 0) return FX_OK;
  const auto set = [hs](void* at, int byte, size_t bytes) { return hipMemsetAsync(at, byte, bytes, hs) == hipSuccess; };
  if (!fx::ts_clear_planes(set, a.out, p->fast_quorum, nullptr)) return FX_ERR_HIP;
  return launch<true>(a, hs) ? FX_OK : FX_ERR_HIP;
}
