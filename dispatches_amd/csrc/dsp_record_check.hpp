// dsp_record_check.hpp — the host-side check of dsp_loop_record's descriptor (ABI 21): plain C++ on the header alone, so that it also
// compiles into a stand-alone program under the host sanitizers (tools/record_check_main.cpp) without the HIP runtime
#pragma once
#include "../../include/dsp_hip.h"

namespace dsp {

// every refusal stated at dsp_loop_record (include/dsp_hip.h): true = safe to launch the gather.  Reads nothing behind a pointer
inline bool loop_record_ok(const dsp_loop_record_desc *d, int32_t B) {
  const int64_t max_stride = (int64_t)1 << 40;
  if (!d || !d->clock || B < 1) return false;
  if (d->n_plants < 1 || d->n_plants > DSP_RECORD_MAX_PLANTS || d->n_segments < 1 || d->n_segments > DSP_RECORD_MAX_SEGMENTS) return false;
  if (d->rows < 1 || d->rows > (1 << 24) || d->divisor < 1 || d->divisor > 8784 || (d->offset != 0 && d->offset != -1) || d->reserved != 0) return false;
  for (int q = 0; q < d->n_plants; ++q)
    if (d->plants[q] < 0 || d->plants[q] >= B || (q > 0 && d->plants[q] <= d->plants[q - 1])) return false;
  for (int g = 0; g < d->n_segments; ++g) {
    const dsp_loop_record_segment &s = d->segments[g];
    if (!s.src || !s.dst || s.width < 1 || s.width > DSP_RECORD_MAX_WIDTH || (s.elem_bytes != 4 && s.elem_bytes != 8)) return false;
    if (s.plant_stride < 1 || s.plant_stride > max_stride || s.elem_stride < 1 || s.elem_stride > max_stride) return false;
  }
  return true;
}

}  // namespace dsp
