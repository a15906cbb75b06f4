// metrics_host.cpp — the host twin of graph_metrics.hip: fx_batch_metrics_host
// (fx_metrics.h holds what the two sides share; the semantics, row by row:
// fantoch_amd.h).  No HIP call in here, so the file also builds alone with a
// host compiler (tests/cpp/metrics_host_check.cpp under the sanitizers).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the function attributes of fx_synth.h
#endif
#include <algorithm>
#include <thread>
#include <vector>

#include "fx_metrics.h"

namespace {

// the samples of stream s, counted into chain[nbins_chain] and delay[nbins_delay]
void stream_samples(const fx_stream_batch& in, const fx_order_batch& out, uint32_t s, uint64_t* chain, uint32_t nbc,
                    uint64_t* delay, uint32_t nbd) {
  const uint32_t steps = in.steps;
  const uint32_t ne = fx::metrics_rows(out.nexec[s], steps);
  for (uint32_t k = 0; k < ne; ++k) {
    const uint32_t o = out.order[fx_index(k, s, steps)];
    const uint32_t rec = FX_ORDER_REC(o);
    if (rec >= steps) continue;
    const uint32_t rs = out.release[fx_index(rec, s, steps)];
    if (rs >= steps) continue;  // not executed (FX_RELEASE_NONE), or no row
    const uint32_t dl = FX_HDR_T(in.hdr[fx_index(rs, s, steps)]) - FX_HDR_T(in.hdr[fx_index(rec, s, steps)]);
    ++delay[fx::metrics_bin(dl, nbd)];
    if (o & FX_ORDER_SCC_START) {
      uint32_t size = 1;
      while (k + size < ne && !(out.order[fx_index(k + size, s, steps)] & FX_ORDER_SCC_START)) ++size;
      ++chain[fx::metrics_bin(size, nbc)];
    }
  }
}

}  // namespace

extern "C" int fx_batch_metrics_host(const fx_stream_batch* in, const fx_order_batch* out, const fx_hist_batch* h) {
  const int st = fx::metrics_check(in, out, h);
  if (st) return st;
  const uint32_t S = in->num_streams, nbc = h->nbins_chain, nbd = h->nbins_delay;
  if (S == 0u || in->steps == 0u) return FX_OK;
  // streams are independent: up to 16 threads, each a contiguous share counted
  // into histograms of its own, added to the caller's once all are done
  const uint32_t nt = S < 64 ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (nt == 1) {
    for (uint32_t s = 0; s < S; ++s) stream_samples(*in, *out, s, h->chain_size, nbc, h->execution_delay, nbd);
    return FX_OK;
  }
  std::vector<std::vector<uint64_t>> part(nt, std::vector<uint64_t>((size_t)nbc + nbd, 0u));
  auto share = [&](uint32_t t) {
    uint64_t* const mine = part[t].data();
    for (uint32_t s = (uint32_t)((uint64_t)S * t / nt); s < (uint32_t)((uint64_t)S * (t + 1) / nt); ++s)
      stream_samples(*in, *out, s, mine, nbc, mine + nbc, nbd);
  };
  std::vector<std::thread> th;
  for (uint32_t t = 0; t < nt; ++t) th.emplace_back(share, t);
  for (auto& x : th) x.join();
  for (uint32_t t = 0; t < nt; ++t) {
    for (uint32_t q = 0; q < nbc; ++q) h->chain_size[q] += part[t][q];
    for (uint32_t q = 0; q < nbd; ++q) h->execution_delay[q] += part[t][nbc + q];
  }
  return FX_OK;
}
