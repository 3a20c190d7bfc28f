// dsp_loop.hip — the hand-off kernels of the rolling double loops, gfx950 only (dsp_wb_rolling_update, dsp_loop_update, dsp_loop_ledger: dsp_capi_loop.hip)
#include <hip/hip_runtime.h>

#include "dsp_device.hpp"
#include "dsp_loop_device.hpp"

using namespace dsp;

// ---- rolling-horizon hand-off of the wind + battery double loop: one thread per plant ------------------------------------------
// Every product is made opaque to the optimiser before it is added (loop_opaque, dsp_loop_device.hpp: no FMA contraction - the _rn
// intrinsics are plain operators to the compiler and `#pragma clang fp contract(off)` did not keep it from fusing them): the results are
// bit-identical to the element-wise tensor operations this kernel replaces (dispatches_amd/rolling.py, use_fused=False),
// which is how it is tested.
// outcome of the solve that has just finished, folded into the loop's device-side flags (what six tensor launches per solve did)
template <class M, class S>
__device__ __forceinline__ void loop_check(const S &s, const M &m, int b) {
  if (m.status && s.bad && m.status[b] != 0) *s.bad = 1;
  if (m.flags && s.uncertified && (m.flags[b] & DSP_FLAG_OBJ_WAIVED)) atomicAdd(reinterpret_cast<unsigned long long *>(s.uncertified), 1ull);
}

__global__ void __launch_bounds__(256) wb_rolling_kernel(dsp_wb_state s, dsp_wb_model rt, dsp_wb_model tr, int phase, int k) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= s.B) return;
  const long long h = *s.hour, st0 = s.start[b];
  auto win = [&](const double *series, int t) { return series[(st0 + h + t) % s.N]; };
  if (phase == 0) {
    const dsp_wb_model &m = rt;
    const int known = min(m.T, 24 - k);
    double *c = m.c + (size_t)b * m.n, *lb = m.lb + (size_t)b * m.n, *ub = m.ub + (size_t)b * m.n;
    double avail_sum = 0.0;
    for (int t = 0; t < m.T; ++t) {
      const double rtp = win(s.rt_series, t);
      const double dap = t < known ? s.da_prices[(size_t)b * 24 + k + t] : win(s.da_series, t);
      const double r3 = loop_opaque(__dmul_rn(1e-3, rtp));
      c[m.pt_cols[t][0]] = __dsub_rn(m.base_c[m.pt_cols[t][0]], r3);
      c[m.pt_cols[t][1]] = __dsub_rn(m.base_c[m.pt_cols[t][1]], r3);
      c[m.pda_cols[t]] = __dsub_rn(m.base_c[m.pda_cols[t]], loop_opaque(__dsub_rn(dap, rtp)));
      const double avail = __dmul_rn(m.wind_kw, win(s.cf_series, t));
      ub[m.wind_cols[t]] = avail;
      avail_sum = t ? __dadd_rn(avail_sum, avail) : avail;
      const double fix = t < known ? s.da_offer[(size_t)b * 24 + k + t] : 0.0;
      lb[m.pda_cols[t]] = fix;
      ub[m.pda_cols[t]] = t < known ? fix : INFINITY;
    }
    if (m.c0) m.c0[b] = __dadd_rn(m.c0_base, loop_opaque(__dmul_rn(m.waste_per_kw, avail_sum)));
    lb[m.soc_init] = s.soc[b]; ub[m.soc_init] = s.soc[b];
    lb[m.thr_init] = s.thr[b]; ub[m.thr_init] = s.thr[b];
  } else if (phase == 1) {
    loop_check(s, rt, b);
    const double *xr = rt.x + (size_t)b * rt.n;
    double *lb = tr.lb + (size_t)b * tr.n, *ub = tr.ub + (size_t)b * tr.n;
    double *rlo = tr.rlo + (size_t)b * tr.m, *rhi = tr.rhi + (size_t)b * tr.m;
    double avail_sum = 0.0;
    for (int t = 0; t < tr.T; ++t) {
      const double offer = __dmul_rn(1e-3, loop_opaque(__dadd_rn(xr[rt.pt_cols[t][0]], xr[rt.pt_cols[t][1]])));
      rlo[tr.track_rows[t]] = offer;
      rhi[tr.track_rows[t]] = offer;
      const double avail = __dmul_rn(tr.wind_kw, win(s.cf_series, t));
      ub[tr.wind_cols[t]] = avail;
      avail_sum = t ? __dadd_rn(avail_sum, avail) : avail;
    }
    if (tr.c0) tr.c0[b] = __dadd_rn(tr.c0_base, loop_opaque(__dmul_rn(tr.waste_per_kw, avail_sum)));
    lb[tr.soc_init] = s.soc[b]; ub[tr.soc_init] = s.soc[b];
    lb[tr.thr_init] = s.thr[b]; ub[tr.thr_init] = s.thr[b];
  } else {
    loop_check(s, tr, b);
    const double *x = tr.x + (size_t)b * tr.n;
    const double delivered = loop_opaque(__dmul_rn(1e-3, loop_opaque(__dadd_rn(x[tr.pt_cols[0][0]], x[tr.pt_cols[0][1]]))));
    const double rt0 = win(s.rt_series, 0);
    s.delivered[b] = delivered;
    s.soc[b] = __ddiv_rn(rint(loop_opaque(__dmul_rn(x[tr.soc0], 100.0))), 100.0);
    s.thr[b] = __ddiv_rn(rint(loop_opaque(__dmul_rn(x[tr.thr0], 100.0))), 100.0);
    const double dao = s.da_offer[(size_t)b * 24 + k], dap = s.da_prices[(size_t)b * 24 + k];
    const double t1 = loop_opaque(__dmul_rn(delivered, rt0)), t2 = loop_opaque(__dmul_rn(dao, loop_opaque(__dsub_rn(dap, rt0))));
    s.revenue[b] = __dadd_rn(s.revenue[b], loop_opaque(__dadd_rn(t1, t2)));
    s.energy_mwh[b] = __dadd_rn(s.energy_mwh[b], delivered);
  }
}

// the clock advances AFTER every plant has read it (own launch: stream order is the barrier)
__global__ void wb_clock_kernel(long long *hour) { *hour += 1; }

// ---- the same hand-off for a flowsheet given by a descriptor (include/dsp_hip.h: dsp_loop_model / dsp_loop_state) ------------------------
__device__ __forceinline__ double loop_power(const dsp_loop_model &m, const double *x, int t) {
  double p = m.pt_const[t];
  if (m.pt_cols[t][0] >= 0) p = fma(m.pt_coef[t][0], x[m.pt_cols[t][0]], p);
  if (m.pt_cols[t][1] >= 0) p = fma(m.pt_coef[t][1], x[m.pt_cols[t][1]], p);
  return p;
}
__device__ __forceinline__ void loop_state_and_wind(const dsp_loop_state &s, const dsp_loop_model &m, int b, long long h, long long st0, double c0) {
  double *lb = m.lb + (size_t)b * m.n, *ub = m.ub + (size_t)b * m.n;
  for (int j = 0; j < m.n_state; ++j) {
    const double v = s.state[(size_t)b * m.n_state + j];
    lb[m.state_init[j]] = v; ub[m.state_init[j]] = v;
  }
  if (m.wind_cols[0] >= 0) {
    const double kw = m.wind_kw_plant ? m.wind_kw_plant[b] : m.wind_kw;     // per-plant size (ABI 16) at the site of the scalar
    double sum = 0.0;
    for (int t = 0; t < m.T; ++t) {
      const double avail = kw * s.cf_series[(st0 + h + t) % s.N];
      ub[m.wind_cols[t]] = avail;
      sum += avail;
    }
    c0 = fma(m.waste_per_kw, sum, c0);
  }
  m.c0[b] = c0;
}
__global__ void __launch_bounds__(256) loop_update_kernel(dsp_loop_state s, dsp_loop_model rt, dsp_loop_model tr, int phase, int k) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= s.B) return;
  const long long h = *s.hour, st0 = s.start[b];
  auto win = [&](const double *series, int t) { return series[(st0 + h + t) % s.N]; };
  if (phase == 0) {
    const dsp_loop_model &m = rt;
    const int known = min(m.T, 24 - k);
    double *c = m.c + (size_t)b * m.n, *lb = m.lb + (size_t)b * m.n, *ub = m.ub + (size_t)b * m.n;
    double c0 = m.c0_base_plant ? m.c0_base_plant[b] : m.c0_base;
    for (int t = 0; t < m.T; ++t) {
      const double rtp = win(s.rt_series, t);
      const double dap = t < known ? s.da_prices[(size_t)b * 24 + k + t] : win(s.da_series, t);
      for (int e = 0; e < 2; ++e)
        if (m.pt_cols[t][e] >= 0) c[m.pt_cols[t][e]] = fma(-rtp, m.pt_coef[t][e], m.base_c[m.pt_cols[t][e]]);
      c[m.pda_cols[t]] = m.base_c[m.pda_cols[t]] - (dap - rtp);
      c0 = fma(-rtp, m.pt_const[t], c0);
      const double fix = t < known ? s.da_offer[(size_t)b * 24 + k + t] : 0.0;
      lb[m.pda_cols[t]] = fix;
      ub[m.pda_cols[t]] = t < known ? fix : INFINITY;
    }
    loop_state_and_wind(s, m, b, h, st0, c0);
  } else if (phase == 1) {
    loop_check(s, rt, b);
    const double *xr = rt.x + (size_t)b * rt.n;
    double *rlo = tr.rlo + (size_t)b * tr.m, *rhi = tr.rhi + (size_t)b * tr.m;
    for (int t = 0; t < tr.T; ++t) {
      const double rhs = loop_power(rt, xr, t) - tr.pt_const[t];       // real-time offer = SCED dispatch in the stub market
      rlo[tr.track_rows[t]] = rhs;
      rhi[tr.track_rows[t]] = rhs;
    }
    loop_state_and_wind(s, tr, b, h, st0, tr.c0_base_plant ? tr.c0_base_plant[b] : tr.c0_base);
  } else {
    loop_check(s, tr, b);
    const double *x = tr.x + (size_t)b * tr.n;
    const double delivered = loop_power(tr, x, 0);
    const double rt0 = win(s.rt_series, 0);
    s.delivered[b] = delivered;
    for (int j = 0; j < tr.n_state; ++j)                              // implemented profile -> next hour's state, rounded as update_model does
      s.state[(size_t)b * tr.n_state + j] = rint(x[tr.state_real[j]] * s.state_scale[j]) / s.state_scale[j];
    const double dao = s.da_offer[(size_t)b * 24 + k], dap = s.da_prices[(size_t)b * 24 + k];
    s.revenue[b] += delivered * rt0 + dao * (dap - rt0);
    s.energy_mwh[b] += delivered;
  }
}

// ---- the ledger of the implemented hour (dsp_loop_ledger, ABI 20): one lane per (form, plant), plant fastest -----------------------------
// blockIdx.y is the form, so everything a lane reads from the descriptor is wave-uniform and the accumulator traffic of a wave is 64
// consecutive doubles.  Runs between the tracking solve and phase 2 above: the clock is still the implemented hour's.
__global__ void __launch_bounds__(256) loop_ledger_kernel(dsp_loop_state s, const double *x, int n, double wind_kw, const double *wind_kw_plant,
                                                          dsp_loop_ledger_desc g) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
  if (b >= s.B) return;
  const double per_avail = g.per_avail[f];
  double avail0 = 0.0;
  if (per_avail != 0.0) {
    const double kw = wind_kw_plant ? wind_kw_plant[b] : wind_kw;
    avail0 = loop_opaque(__dmul_rn(kw, s.cf_series[(s.start[b] + *s.hour) % s.N]));
  }
  const double *coef = g.coef + (size_t)b * g.coef_stride + f * DSP_LEDGER_MAX_TERMS;
  const double v = loop_ledger_form(x + (size_t)b * n, g.cols[f], coef, g.n_terms[f], g.constant[(size_t)b * g.const_stride + f], per_avail, avail0);
  const size_t at = (size_t)f * s.B + b;
  g.hour_value[at] = v;
  g.acc[at] = __dadd_rn(g.acc[at], loop_opaque(v));
}

// ---- the recorder of the descriptor loop (dsp_loop_record, ABI 21): one lane per element (recorded plant q, element j), j fastest ---------
// A pure gather.  blockIdx.y is the segment, so the segment's fields and the row are wave-uniform; consecutive lanes take consecutive j
// of one plant, so a wave's stores are consecutive and its loads are wherever elem_stride == 1.  The row comes from the device clock:
// whatever falls outside [0, rows) - past the span, or the hour before hour 0 - goes to the spare row `rows`.
__global__ void __launch_bounds__(256) loop_record_kernel(dsp_loop_record_desc d) {
  const dsp_loop_record_segment &g = d.segments[blockIdx.y];
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= d.n_plants * g.width) return;
  const int q = e / g.width, j = e - q * g.width;
  const long long t = *d.clock + d.offset;
  const long long r = (t < 0 || t / d.divisor >= d.rows) ? d.rows : t / d.divisor;
  const size_t from = (size_t)d.plants[q] * (size_t)g.plant_stride + (size_t)j * (size_t)g.elem_stride;
  const size_t to = ((size_t)r * d.n_plants + q) * g.width + j;
  if (g.elem_bytes == 8)
    ((unsigned long long *)g.dst)[to] = ((const unsigned long long *)g.src)[from];
  else
    ((unsigned int *)g.dst)[to] = ((const unsigned int *)g.src)[from];
}

namespace dsp {

// the grid's x spans the widest segment; a narrower one leaves its surplus blocks idle (they return at once)
hipError_t launch_loop_record(const dsp_loop_record_desc &rec, hipStream_t stream) {
  int widest = 0;
  for (int g = 0; g < rec.n_segments; ++g) widest = rec.segments[g].width > widest ? rec.segments[g].width : widest;
  const long long lanes = (long long)rec.n_plants * widest;
  hipLaunchKernelGGL(loop_record_kernel, dim3((unsigned)((lanes + 255) / 256), rec.n_segments), dim3(256), 0, stream, rec);
  return hipGetLastError();
}

hipError_t launch_loop_ledger(const dsp_loop_state &st, const dsp_loop_model &tr, const dsp_loop_ledger_desc &ledger, hipStream_t stream) {
  hipLaunchKernelGGL(loop_ledger_kernel, dim3((st.B + 255) / 256, ledger.n_forms), dim3(256), 0, stream, st, tr.x, (int)tr.n, tr.wind_kw,
                     tr.wind_kw_plant, ledger);
  return hipGetLastError();
}

// one thread per plant; phase 2 is followed by the clock's own launch
template <class K, class S, class M>
static hipError_t launch_hand_off(K kernel, const S &st, const M &rt, const M &tr, int phase, int k, hipStream_t stream) {
  hipLaunchKernelGGL(kernel, dim3((st.B + 255) / 256), dim3(256), 0, stream, st, rt, tr, phase, k);
  if (phase == 2) hipLaunchKernelGGL(wb_clock_kernel, dim3(1), dim3(1), 0, stream, (long long *)st.hour);
  return hipGetLastError();
}
hipError_t launch_wb_rolling(const dsp_wb_state &st, const dsp_wb_model &rt, const dsp_wb_model &tr, int phase, int k, hipStream_t stream) {
  return launch_hand_off(wb_rolling_kernel, st, rt, tr, phase, k, stream);
}
hipError_t launch_loop_update(const dsp_loop_state &st, const dsp_loop_model &rt, const dsp_loop_model &tr, int phase, int k, hipStream_t stream) {
  return launch_hand_off(loop_update_kernel, st, rt, tr, phase, k, stream);
}

}  // namespace dsp
