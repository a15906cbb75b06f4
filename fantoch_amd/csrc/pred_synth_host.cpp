// pred_synth_host.cpp — the host twin of the Caesar commit-stream generator
// (fx_pred_synth.h's pred_synth_emit, one command at a time) and the shape.
// No HIP call in here, so the file also builds alone with a host compiler
// (tests/cpp/pred_synth_host_check.cpp under the sanitizers).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the function attributes of fx_synth.h
#endif
#include <stdint.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "fantoch_amd.h"
#include "fx_pred_synth.h"

using namespace fx;

extern "C" {

int fx_pred_synth_shape(const fx_pred_synth_params* p, uint32_t* num_streams, uint32_t* steps, uint32_t* dmax) {
  return pred_synth_check(p, num_streams, steps, dmax);
}

int fx_pred_synth_generate_host(const fx_pred_synth_params* p, const fx_pred_synth_planes* planes) {
  uint32_t S, steps, dmax;
  int st = pred_synth_check(p, &S, &steps, &dmax);
  if (st) return st;
  st = pred_synth_check_planes(planes, dmax);
  if (st) return st;
  // every command writes its own words of the planes: commands split over threads
  const size_t total = (size_t)p->instances * steps;
  const uint32_t nt = total < 4096 ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  auto work = [&](uint32_t t) {
    for (size_t i = t; i < total; i += nt)
      pred_synth_emit(*p, (uint32_t)(i / steps), (uint32_t)(i % steps), S, steps, dmax, *planes);
  };
  if (nt == 1) {
    work(0);
    return FX_OK;
  }
  std::vector<std::thread> th;
  for (uint32_t t = 0; t < nt; ++t) th.emplace_back(work, t);
  for (auto& x : th) x.join();
  return FX_OK;
}

}  // extern "C"
