// dsp_days_check.hpp — the host-side checks of dsp_loop_profile and of the representative-day entry points (dsp_days_assign,
// dsp_days_update, dsp_days_frequency; added under ABI 22): plain C++ on the header alone, so that they also compile into a stand-alone
// program under the host sanitizers (tools/days_check_main.cpp) without the HIP runtime.  Every function reads the descriptor and the
// pointers' VALUES only, never anything behind a pointer.
#pragma once
#include "../../include/dsp_hip.h"

namespace dsp {

// every refusal stated at dsp_loop_profile: true = safe to launch (or B == 0: nothing to launch)
inline bool loop_profile_ok(const dsp_loop_profile_desc *p) {
  if (!p || !p->clock || !p->delivered || !p->profile) return false;
  if (p->B < 0 || p->B > DSP_DAYS_MAX_PLANTS || p->days < 1 || p->days > DSP_DAYS_MAX_DAYS) return false;
  for (int q = 0; q < 4; ++q)
    if (p->reserved[q] != 0) return false;
  return true;
}

// the descriptor's share of every refusal stated above dsp_days_assign
inline bool days_desc_ok(const dsp_days_desc *d) {
  if (!d || !d->profile || !d->p_min || !d->p_max) return false;
  if (d->B < 0 || d->B > DSP_DAYS_MAX_PLANTS || d->days < 1 || d->days > DSP_DAYS_MAX_DAYS) return false;
  if ((int64_t)d->B * (int64_t)d->days > (int64_t)DSP_DAYS_MAX_POINTS) return false;
  if (d->channels < 1 || d->channels > 2 || d->filter < 0 || d->filter > 1) return false;
  if (d->channels == 2 && (!d->cf_series || !d->start || d->N < 1)) return false;
  for (int q = 0; q < 4; ++q)
    if (d->reserved[q] != 0) return false;
  return true;
}

inline bool days_k_ok(int32_t K) { return K >= 1 && K <= DSP_DAYS_MAX_K; }

// doubles of dsp_days_update's work buffer: one row of K * F sums, K counts, the dist2 sum and the labelled points per chunk of DSP_DAYS_CHUNK points
inline int64_t days_work_doubles(int64_t points, int32_t K, int32_t channels) {
  if (points < 0 || points > (int64_t)DSP_DAYS_MAX_POINTS || !days_k_ok(K) || channels < 1 || channels > 2) return -1;
  const int64_t chunks = (points + DSP_DAYS_CHUNK - 1) / DSP_DAYS_CHUNK;
  return chunks * ((int64_t)K * 24 * channels + K + 2);
}

inline bool days_assign_ok(const dsp_days_desc *d, const double *centers, int32_t K, const int32_t *label, const double *dist2) {
  return days_desc_ok(d) && days_k_ok(K) && centers && label && dist2;
}

inline bool days_update_ok(const dsp_days_desc *d, const int32_t *label, const double *dist2, int32_t K, const double *centers,
                           const int64_t *count, const double *inertia, const double *work, int64_t work_doubles) {
  if (!days_desc_ok(d) || !days_k_ok(K) || !label || !dist2 || !centers || !count || !inertia || !work) return false;
  return work_doubles >= days_work_doubles((int64_t)d->B * d->days, K, d->channels);
}

inline bool days_frequency_ok(const dsp_days_desc *d, const int32_t *label, int32_t K, const double *freq) {
  return days_desc_ok(d) && days_k_ok(K) && label && freq;
}

}  // namespace dsp
