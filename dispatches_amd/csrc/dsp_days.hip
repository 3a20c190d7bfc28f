// dsp_days.hip — day profiles of the descriptor double loop and the representative days over them, gfx950 only (include/dsp_hip.h:
// dsp_loop_profile, dsp_days_assign, dsp_days_update, dsp_days_frequency, added under ABI 22; rolling_flowsheets.py::
// BatchedDoubleLoop(profiles=days), representative_days.py::DayPoints).  The reference's workflow downstream of its double-loop sweeps
// (dispatches/workflow/train_market_surrogates/dynamic/) scales every simulated year to a capacity factor, cuts it into days, sets
// all-zero and all-full days aside, clusters the rest into K representative days and labels every simulation with the share of days
// near each centre.  Here the year already sits on the device, plant-minor, and every step is a memory-streaming kernel:
//
//   loop_profile_kernel   one lane per plant: profile[row of the clock][b] = delivered[b].  One load, one store; nothing else.
//   days_assign_kernel    one lane per (day, plant) point, plants fastest, so the 24 loads of a wave are 24 runs of consecutive doubles.
//                         The point (24 or 48 features) stays in registers; the K <= 64 centres are staged once per workgroup in LDS and
//                         every lane reads the same address (a broadcast).  Writes the nearest centre and the squared distance.
//   days_partial_kernel   one wave per chunk of DSP_DAYS_CHUNK points; lane j < F owns feature j, lane F the member counts, lane F + 1
//                         the dist2 sum and the labelled points.  The wave walks its points in the order of p and each lane adds into
//                         its own column of an LDS table [K][F]: a fixed order, no atomics, no cross-lane traffic.
//   days_combine_kernel   one lane per entry of that table: the chunks added in chunk order, centre = sum / count.
//   days_frequency_kernel one lane per plant walks its labels; K + 2 integer counters per lane in LDS ([slot][lane]: lane-minor, so a
//                         wave's accesses to one slot fall on 64 different banks), one division per entry.
//
// Every operation of a point is rounded on its own (the _rn intrinsics) and a product is opaque before a sum takes it (loop_opaque: no
// fma contraction), in a stated order: representative_days.py restates scale, class, assign, update and frequency in numpy, and the
// kernels are tested against that bit for bit.  The host entry points check every pointer and size (dsp_days_check.hpp) before they
// launch: a lane indexes [0, days * 24 * B) of the profile, [0, B) of the per-plant arrays, [0, N) of the series (the index is reduced
// mod N and made non-negative whatever `start` holds), [0, K * F) of the centres and its own chunk row of the work buffer.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dsp_hip.h"
#include "dsp_capi_internal.hpp"
#include "dsp_days_check.hpp"
#include "dsp_loop_device.hpp"

using dsp::loop_opaque;

static_assert(sizeof(dsp_days_desc) + 64 <= 4096 && sizeof(dsp_loop_profile_desc) <= 4096, "the descriptors travel as by-value kernel arguments: HIP's limit is 4 KB");

__global__ void __launch_bounds__(256) loop_profile_kernel(dsp_loop_profile_desc p) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  const long long h = *p.clock - 1;
  long long day = h / 24, hod = h % 24;
  if (h < 0) { day = p.days; hod = 0; }
  if (day > p.days) day = p.days;
  p.profile[(size_t)(day * 24 + hod) * (size_t)p.B + (size_t)b] = p.delivered[b];
}

// feature j of point (day, b): the scaled dispatch of hour j, or (j >= 24) the realised capacity factor of hour j - 24
__device__ __forceinline__ double days_feature(const dsp_days_desc &d, int day, int b, int j, double lo, double span) {
  if (j < 24) return __ddiv_rn(__dsub_rn(d.profile[((size_t)day * 24 + (size_t)j) * (size_t)d.B + (size_t)b], lo), span);
  long long at = (d.start[b] + 24ll * day + (j - 24)) % d.N;
  if (at < 0) at += d.N;
  return d.cf_series[at];
}

template <int CH>
__global__ void __launch_bounds__(256) days_assign_kernel(dsp_days_desc d, const double *centers, int K, int32_t *label, double *dist2) {
  constexpr int F = 24 * CH;
  __shared__ double c[DSP_DAYS_MAX_K * F];
  for (int i = threadIdx.x; i < K * F; i += 256) c[i] = centers[i];
  __syncthreads();
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)d.B * d.days) return;
  const int b = (int)(p % d.B), day = (int)(p / d.B);
  const double lo = d.p_min[b], span = __dsub_rn(d.p_max[b], lo);
  double x[F];
#pragma unroll
  for (int j = 0; j < F; ++j) x[j] = days_feature(d, day, b, j, lo, span);
  int lab = 0;
  double best = 0.0;
  if (d.filter) {
    double s = x[0];
#pragma unroll
    for (int h = 1; h < 24; ++h) s = __dadd_rn(s, x[h]);
    lab = s == 0.0 ? -1 : s == 24.0 ? -2 : 0;
  }
  if (lab == 0) {
    for (int k = 0; k < K; ++k) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < F; ++j) {
        const double dd = __dsub_rn(x[j], c[k * F + j]);
        acc = __dadd_rn(acc, loop_opaque(__dmul_rn(dd, dd)));
      }
      if (k == 0 || acc < best) { best = acc; lab = k; }
    }
  }
  label[p] = lab;
  dist2[p] = best;
}

template <int CH>
__global__ void __launch_bounds__(64) days_partial_kernel(dsp_days_desc d, const int32_t *label, const double *dist2, int K, double *work) {
  constexpr int F = 24 * CH;
  __shared__ double acc[DSP_DAYS_MAX_K * F + DSP_DAYS_MAX_K + 2];
  const int row = K * F + K + 2, j = threadIdx.x;
  for (int i = j; i < row; i += 64) acc[i] = 0.0;
  __syncthreads();
  const long long P = (long long)d.B * d.days, p0 = (long long)blockIdx.x * DSP_DAYS_CHUNK;
  const long long p1 = p0 + DSP_DAYS_CHUNK < P ? p0 + DSP_DAYS_CHUNK : P;
  int b = (int)(p0 % d.B), day = (int)(p0 / d.B);
  for (long long p = p0; p < p1; ++p) {
    const int lab = label[p];                        // (the same address in every lane: the branch is uniform)
    if (lab >= 0 && lab < K) {
      if (j < F) {
        const double lo = d.p_min[b], span = __dsub_rn(d.p_max[b], lo);
        acc[lab * F + j] = __dadd_rn(acc[lab * F + j], days_feature(d, day, b, j, lo, span));
      } else if (j == F) {
        acc[K * F + lab] += 1.0;
      } else if (j == F + 1) {
        acc[K * F + K] = __dadd_rn(acc[K * F + K], dist2[p]);
        acc[K * F + K + 1] += 1.0;
      }
    }
    if (++b == d.B) { b = 0; ++day; }
  }
  __syncthreads();
  for (int i = j; i < row; i += 64) work[(size_t)blockIdx.x * (size_t)row + (size_t)i] = acc[i];
}

__global__ void __launch_bounds__(256) days_combine_kernel(int K, int F, long long chunks, const double *work, double *centers, int64_t *count,
                                                           double *inertia) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, row = K * F + K + 2;
  if (i >= K * F + K + 1) return;
  const int n_at = i < K * F ? K * F + i / F : i < K * F + K ? i : K * F + K + 1;      // the count that belongs to entry i
  double s = 0.0, n = 0.0;
  for (long long q = 0; q < chunks; ++q) {
    s = __dadd_rn(s, work[(size_t)q * (size_t)row + (size_t)i]);
    n += work[(size_t)q * (size_t)row + (size_t)n_at];                                   // (integers below 2^31: exact)
  }
  if (i < K * F) {
    if (n > 0.0) centers[i] = __ddiv_rn(s, n);
  } else if (i < K * F + K) {
    count[i - K * F] = (int64_t)n;
  } else {
    *inertia = n > 0.0 ? __ddiv_rn(s, n) : 0.0;
  }
}

__global__ void __launch_bounds__(64) days_frequency_kernel(dsp_days_desc d, const int32_t *label, int K, double *freq) {
  __shared__ int32_t cnt[(DSP_DAYS_MAX_K + 2) * 64];
  const int lane = threadIdx.x, b = blockIdx.x * 64 + lane, slots = d.filter ? K + 2 : K;
  for (int s = 0; s < slots; ++s) cnt[s * 64 + lane] = 0;          // (a lane's own column: no barrier needed)
  if (b >= d.B) return;
  for (int day = 0; day < d.days; ++day) {
    const int lab = label[(size_t)day * (size_t)d.B + (size_t)b];
    int s = -1;
    if (lab >= 0 && lab < K) s = d.filter ? lab + 1 : lab;
    else if (d.filter && lab == -1) s = 0;
    else if (d.filter && lab == -2) s = K + 1;
    if (s >= 0) cnt[s * 64 + lane] += 1;
  }
  const double days = (double)d.days;
  for (int s = 0; s < slots; ++s) freq[(size_t)b * (size_t)slots + (size_t)s] = __ddiv_rn((double)cnt[s * 64 + lane], days);
}

extern "C" int dsp_loop_profile(const dsp_loop_profile_desc *p, void *hipStream) {
  if (!dsp::loop_profile_ok(p)) return DSP_ERR_INVALID;
  if (p->B == 0) return DSP_OK;
  hipLaunchKernelGGL(loop_profile_kernel, dim3((unsigned)((p->B + 255) / 256)), dim3(256), 0, (hipStream_t)hipStream, *p);
  HIP_TRY(hipGetLastError());
  return DSP_OK;
}

extern "C" int64_t dsp_days_work_doubles(int64_t points, int32_t K, int32_t channels) { return dsp::days_work_doubles(points, K, channels); }

extern "C" int dsp_days_assign(const dsp_days_desc *d, const double *centers, int32_t K, int32_t *label, double *dist2, void *hipStream) {
  if (!dsp::days_assign_ok(d, centers, K, label, dist2)) return DSP_ERR_INVALID;
  if (d->B == 0) return DSP_OK;
  const long long P = (long long)d->B * d->days;
  const dim3 grid((unsigned)((P + 255) / 256)), block(256);
  if (d->channels == 1)
    hipLaunchKernelGGL(days_assign_kernel<1>, grid, block, 0, (hipStream_t)hipStream, *d, centers, (int)K, label, dist2);
  else
    hipLaunchKernelGGL(days_assign_kernel<2>, grid, block, 0, (hipStream_t)hipStream, *d, centers, (int)K, label, dist2);
  HIP_TRY(hipGetLastError());
  return DSP_OK;
}

extern "C" int dsp_days_update(const dsp_days_desc *d, const int32_t *label, const double *dist2, int32_t K, double *centers, int64_t *count,
                               double *inertia, double *work, int64_t work_doubles, void *hipStream) {
  if (!dsp::days_update_ok(d, label, dist2, K, centers, count, inertia, work, work_doubles)) return DSP_ERR_INVALID;
  if (d->B == 0) return DSP_OK;
  const long long P = (long long)d->B * d->days, chunks = (P + DSP_DAYS_CHUNK - 1) / DSP_DAYS_CHUNK;
  const int F = 24 * d->channels;
  if (d->channels == 1)
    hipLaunchKernelGGL(days_partial_kernel<1>, dim3((unsigned)chunks), dim3(64), 0, (hipStream_t)hipStream, *d, label, dist2, (int)K, work);
  else
    hipLaunchKernelGGL(days_partial_kernel<2>, dim3((unsigned)chunks), dim3(64), 0, (hipStream_t)hipStream, *d, label, dist2, (int)K, work);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(days_combine_kernel, dim3((unsigned)((K * F + K + 1 + 255) / 256)), dim3(256), 0, (hipStream_t)hipStream, (int)K, F, chunks,
                     (const double *)work, centers, count, inertia);
  HIP_TRY(hipGetLastError());
  return DSP_OK;
}

extern "C" int dsp_days_frequency(const dsp_days_desc *d, const int32_t *label, int32_t K, double *freq, void *hipStream) {
  if (!dsp::days_frequency_ok(d, label, K, freq)) return DSP_ERR_INVALID;
  if (d->B == 0) return DSP_OK;
  hipLaunchKernelGGL(days_frequency_kernel, dim3((unsigned)((d->B + 63) / 64)), dim3(64), 0, (hipStream_t)hipStream, *d, label, (int)K, freq);
  HIP_TRY(hipGetLastError());
  return DSP_OK;
}
