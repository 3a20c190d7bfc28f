// dsp_param.hip — parametrized two-tier bidding of the descriptor double loop on the device, gfx950 only (include/dsp_hip.h:
// dsp_loop_param_step; rolling_flowsheets.py: BatchedDoubleLoop with bidder="parametrized").
//
// Reference behaviour (run_double_loop_PEM.py with PEMParametrizedBidder, run_double_loop_battery_parametrized.py with
// FixedParametrizedBidder, both on a PerfectForecaster): no bidding LP; the bid curve of an hour is a closed form of the available
// wind w, the storage size and one bid price: (0, 0), (max(0, w - storage), 0), (p_max, bid), p_max = w or max(w, storage).
//
//   param_curve_kernel<DA>   one lane per (plant, period): window index, the three pairs in integer cents (dsp_bid_cents.hpp), the
//                            curve, the clearing.  The pairs are ordered by construction (0 <= max(0, w - s) <= p_max, prices 0, 0,
//                            bid >= 0), so the sort network of the LP bidder's clearing kernel reduces to two compares of cent values:
//                            "is the middle power above 0" and "is the last power above the middle one".  A pair that repeats a
//                            power keeps the higher price, which is the later pair's.  DA = true: 24 hours on the day-ahead capacity
//                            factors and prices; DA = false: the tracker's periods on the real-time ones, and the tracker's LP of
//                            the hour on the cleared dispatch.
//   param_h2_kernel          one lane per plant, after the tracking solve: hydrogen of the implemented hour.
//
// Every product is rounded on its own (__dmul_rn / __dadd_rn / __dsub_rn, and an opaque register between a product and the sum that
// takes it - the intrinsics alone do not stop the compiler from contracting the two into one fma): bit-identical to
// the tensor operations of BatchedDoubleLoop (use_fused=False), which go through workflow/market.py::plant_curves / clear_curves.
// The points of a curve (loop_emit_point, loop_curve_close) and the plant half of the tracker's LP (loop_tracker_plant) are the shared
// ones of dsp_loop_device.hpp.  Vector stores only, no atomics, no LDS; VGPRs / scratch: profiles/loop_device_kernel_resources.txt.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dsp_hip.h"
#include "dsp_device.hpp"
#include "dsp_loop_device.hpp"

#pragma clang fp contract(off)

namespace dsp {

static_assert(sizeof(dsp_loop_param_state) + sizeof(dsp_loop_model) + 64 <= 4096,
              "the descriptors travel as by-value kernel arguments: HIP's limit is 4 KB");

template <bool DA>
__global__ void __launch_bounds__(256) param_curve_kernel(dsp_loop_param_state s, dsp_loop_model tr, int T) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= s.B * T) return;
  const int b = g / T, t = g - b * T;
  const long long h = *s.hour, st0 = s.start[b];
  const long long at = (st0 + h + t) % s.N;
  const double lmp = (DA ? s.da_series : s.rt_series)[at];
  const double bid = s.bid_price[b], storage = s.storage_mw[b];
  // ---- the three pairs: (0, 0), (lo, 0), (hi, bid) ----
  const double w = loop_opaque(__dmul_rn((DA ? s.da_cf_series : s.rt_cf_series)[at], s.wind_mw));      // opaque: w - storage must not become one fma
  const double lo = fmax(__dsub_rn(w, storage), 0.0);
  const double hi = s.battery ? fmax(w, storage) : w;
  const long long lo_c = bid_cents(lo), hi_c = bid_cents(hi), bid_c = bid_cents(bid);
  const bool has_lo = lo_c >= 0 && fabs(lo) < INFINITY;              // a pair takes part with finite numbers and a power >= 0
  const bool has_hi = hi_c >= 0 && fabs(hi) < INFINITY && fabs(bid) < INFINITY;
  // ---- distinct powers ascending, the highest price at each, running maximum; cleared on the way ----
  int32_t *out = (DA ? s.da_curve : s.rt_curve) + (size_t)g * 8;
  int pos = 0;
  long long run = 0, cleared = 0;
  const bool price_taker = s.price_taker != 0;
  auto emit = [&](long long U, long long M) { loop_emit_point(out, pos, run, cleared, U, M, price_taker, lmp); };
  const bool lo_new = has_lo && lo_c > 0;                            // compare 1: the middle pair is a point of its own
  const long long below = lo_new ? lo_c : 0;                         // the largest power in front of the last pair
  const bool hi_new = has_hi && hi_c > below;                        // compare 2: the last pair is a point of its own
  const bool hi_joins = has_hi && hi_c == below;                     // ... or repeats the power in front of it: the higher price stays
  emit(0, (!lo_new && hi_joins) ? max(0ll, bid_c) : 0ll);
  if (lo_new) emit(lo_c, hi_joins ? max(0ll, bid_c) : 0ll);
  if (hi_new) emit(hi_c, bid_c);
  (DA ? s.da_count : s.rt_count)[g] = pos;
  const double disp = loop_curve_close(out, pos, 4, cleared);
  if (DA) {
    s.da_offer[g] = disp;
    s.da_prices[g] = lmp;
    return;
  }
  s.rt_dispatch[g] = disp;
  // ---- the tracker's LP of this hour on the cleared dispatch (one wind size: the host refuses per-plant pointers here) ----
  double *rlo = tr.rlo + (size_t)b * tr.m, *rhi = tr.rhi + (size_t)b * tr.m;
  const double rhs = __dsub_rn(disp, tr.pt_const[t]);
  rlo[tr.track_rows[t]] = rhs;
  rhi[tr.track_rows[t]] = rhs;
  if (t == 0) loop_tracker_plant(tr, b, s.rt_cf_series, st0 + h, s.N, s.state + (size_t)b * tr.n_state);
}

__global__ void __launch_bounds__(256) param_h2_kernel(dsp_loop_param_state s, dsp_loop_model tr) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= s.B) return;
  const double kw = tr.x[(size_t)b * tr.n + s.pem_col];
  const double kg = __dmul_rn(__ddiv_rn(loop_opaque(__dmul_rn(kw, s.h2_mul)), s.h2_div), 3600.0);
  s.h2_kg[b] = __dadd_rn(s.h2_kg[b], loop_opaque(kg));
}

hipError_t launch_loop_param_step(const dsp_loop_param_state &st, const dsp_loop_model &tr, int phase, hipStream_t stream) {
  const dim3 block(256);
  if (phase == 0) {
    const long long lanes = (long long)st.B * 24;
    hipLaunchKernelGGL(param_curve_kernel<true>, dim3((unsigned)((lanes + 255) / 256)), block, 0, stream, st, tr, 24);
  } else if (phase == 1) {
    const long long lanes = (long long)st.B * tr.T;
    hipLaunchKernelGGL(param_curve_kernel<false>, dim3((unsigned)((lanes + 255) / 256)), block, 0, stream, st, tr, (int)tr.T);
  } else {
    hipLaunchKernelGGL(param_h2_kernel, dim3((unsigned)((st.B + 255) / 256)), block, 0, stream, st, tr);
  }
  return hipGetLastError();
}

}  // namespace dsp
