// fx_metrics.h — the metrics pass (host + device): what graph_metrics.hip and
// metrics_host.cpp share: the argument checks, the streams the pass reads, the
// bin of a sample and the size up to which the histograms stay in LDS.
#pragma once
#include <stdint.h>

#include "fx_synth.h"

namespace fx {

// (nbins_chain + nbins_delay) * 4 bytes at or below this: a block counts in
// LDS and adds its bins to the global histograms once; above it every wave
// adds to the global histograms directly
constexpr uint32_t METRICS_LDS_BYTES = 48u * 1024u;

inline int metrics_check(const fx_stream_batch* in, const fx_order_batch* out, const fx_hist_batch* h) {
  if (!in || !out || !h || !h->chain_size || !h->execution_delay || h->nbins_chain < 2 || h->nbins_delay < 2)
    return FX_ERR_INVALID_ARG;
  if (!in->hdr || !out->order || !out->release || !out->nexec) return FX_ERR_INVALID_ARG;
  return FX_OK;
}

// The order rows of a stream the pass reads: nexec[s] of them, none where that
// count cannot be one (above `steps`: a stream no launch wrote, a stopped
// driver), so no row index leaves the plane.
FX_HD uint32_t metrics_rows(uint32_t nexec, uint32_t steps) { return nexec <= steps ? nexec : 0u; }

// The last bin takes every sample from nbins - 1 up.
FX_HD uint32_t metrics_bin(uint32_t sample, uint32_t nbins) { return sample < nbins - 1u ? sample : nbins - 1u; }

}  // namespace fx
