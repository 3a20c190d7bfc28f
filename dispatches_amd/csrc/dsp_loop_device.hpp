// dsp_loop_device.hpp — the device arithmetic that the double-loop kernels share (dsp_market.hip, dsp_param.hip, dsp_project.hip and the
// hand-off kernels of dsp_loop.hip), written once.  Device-only, every function __forceinline__.
//
//   loop_opaque           the register barrier between a product and the sum that takes it: the _rn intrinsics alone do not keep the
//                         compiler from contracting the two into one fma.
//   loop_scenario_index   the Backcaster's index rule into a plant's circular series, for any market state struct.
//   loop_wind_window      wind bounds of a window and their sum;  loop_c0: base + per_kw * sum.  The wind + battery model
//                         (dsp_wb_model) and the descriptor model (dsp_loop_model) share exactly these two.
//   loop_tracker_plant    the plant half of a tracker's LP over a dsp_loop_model: state columns fixed, wind bounds of the window,
//                         objective constant.  The dispatch row of a period stays with the kernel that knows its value.
//   loop_ledger_form      one linear form of the ledger of the implemented hour on the tracker's solution (dsp_loop_ledger).
//   loop_emit_point       one point of a bid curve: running maximum of the price, cleared on the way.
//   loop_curve_close      zero-filled tail of a curve, cleared cents -> MW.
//   loop_curve_and_clear  sorted keys -> curve points, count, tail, cleared dispatch, for a curve that starts at p_min.
//
// Every product is rounded on its own and opaque before a sum takes it, sums run in the order of t: bit-identical to the tensor
// operations of BatchedDoubleLoop / BatchedWindBatteryDoubleLoop (use_fused=False), which is how the kernels are tested.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dsp_hip.h"
#include "dsp_bid_cents.hpp"

namespace dsp {

__device__ __forceinline__ double loop_opaque(double v) { asm volatile("" : "+v"(v)); return v; }

// index into the circular series of the price scenario i of plant (start st0) asked at hour-of-day hod for period t (clock h)
template <class State>
__device__ __forceinline__ long long loop_scenario_index(const State &s, long long st0, long long h, int i, int hod, int t) {
  if (!s.backcast) return (st0 + h + t) % s.N;
  const long long D = s.D, d = h / 24;
  const long long pos = (24 * (D - 1 - i) + hod + t) % (24 * D);
  long long v = (st0 + 24 * (d - D) + pos) % s.N;
  return v < 0 ? v + s.N : v;
}

// ub[wind_cols[q]] = kw * cf[(first + q) % N] for the T periods of a window; returns the sum of the bounds in the order of q
__device__ __forceinline__ double loop_wind_window(double *ub, const int32_t *wind_cols, int T, double kw, const double *cf_series,
                                                   long long first, long long N) {
  double avail_sum = 0.0;
  for (int q = 0; q < T; ++q) {
    const double avail = loop_opaque(__dmul_rn(kw, cf_series[(first + q) % N]));
    ub[wind_cols[q]] = avail;
    avail_sum = q ? __dadd_rn(avail_sum, avail) : avail;
  }
  return avail_sum;
}

__device__ __forceinline__ double loop_c0(double base, double per_kw, double avail_sum) {
  return __dadd_rn(base, loop_opaque(__dmul_rn(per_kw, avail_sum)));
}

// the plant half of the tracker's LP of plant b: state columns fixed to state[0 .. n_state), wind bounds of the window that starts at
// series index `first` (mod N), objective constant.  Per-plant sizes where the model carries them, the scalars otherwise.
// (The state goes first: its pointer is dead before the wind loop, which keeps project_write_kernel at its register count.)
__device__ __forceinline__ void loop_tracker_plant(const dsp_loop_model &tr, int b, const double *cf_series, long long first, long long N,
                                                   const double *state) {
  double *lb = tr.lb + (size_t)b * tr.n, *ub = tr.ub + (size_t)b * tr.n;
  for (int j = 0; j < tr.n_state; ++j) {
    const double v = state[j];
    lb[tr.state_init[j]] = v; ub[tr.state_init[j]] = v;
  }
  double c0 = tr.c0_base_plant ? tr.c0_base_plant[b] : tr.c0_base;
  if (tr.wind_cols[0] >= 0) {
    const double kw = tr.wind_kw_plant ? tr.wind_kw_plant[b] : tr.wind_kw;
    c0 = loop_c0(c0, tr.waste_per_kw, loop_wind_window(ub, tr.wind_cols, tr.T, kw, cf_series, first, N));
  }
  tr.c0[b] = c0;
}

// one linear form of the ledger (dsp_loop_ledger_desc) on a plant's solution x: the constant, E terms folded in by fma in the order of e,
// then the wind available in the hour times its factor - the fixed order that BatchedDoubleLoop._ledger_values states with exact_fma
__device__ __forceinline__ double loop_ledger_form(const double *x, const int32_t *cols, const double *coef, int E, double constant,
                                                   double per_avail, double avail0) {
  double v = constant;
  for (int e = 0; e < E; ++e) v = fma(coef[e], x[cols[e]], v);
  if (per_avail != 0.0) v = fma(per_avail, avail0, v);
  return v;
}

// point `pos` of a curve: (U, running maximum of M) in cents; a price taker is cleared up to the last point whose price the lmp covers
__device__ __forceinline__ void loop_emit_point(int32_t *out, int &pos, long long &run, long long &cleared, long long U, long long M,
                                                bool price_taker, double lmp) {
  run = pos == 0 ? M : max(run, M);
  out[2 * pos] = (int32_t)U;
  out[2 * pos + 1] = (int32_t)run;
  if (pos == 0 || !price_taker || __ddiv_rn((double)run, 100.0) <= lmp) cleared = U;
  ++pos;
}

// the unused slots of a curve of `slots` points are zero; the cleared power in MW
__device__ __forceinline__ double loop_curve_close(int32_t *out, int pos, int slots, long long cleared) {
  for (int q = pos; q < slots; ++q) { out[2 * q] = 0; out[2 * q + 1] = 0; }
  return __ddiv_rn((double)cleared, 100.0);
}

// ascending keys (dsp_bid_cents.hpp; dropped pairs last) of the S pairs of a lane -> its curve of S + 1 slots: the distinct powers in
// order with the running maximum of the price, in front of them the p_min point at the lowest price unless a pair sits on it; the
// number of points; the cleared dispatch in MW
template <int SP>
__device__ __forceinline__ double loop_curve_and_clear(const long long (&keys)[SP], int S, long long pmin, bool price_taker, double lmp,
                                                       int32_t *out, int32_t *count) {
  const bool has_min = keys[0] != kBidDrop && bid_key_power(keys[0]) == pmin;      // powers are >= p_min and ascending
  long long lowest = 0x7fffffffffffffffll;
  int n = 0;
#pragma unroll
  for (int i = 0; i < SP; ++i) {
    const bool first = keys[i] != kBidDrop && (i == 0 || bid_key_power(keys[i]) != bid_key_power(keys[i ? i - 1 : 0]));
    if (first) { lowest = min(lowest, bid_key_price(keys[i])); ++n; }
  }
  int pos = 0;
  long long run = 0, cleared = 0;
  if (!has_min) loop_emit_point(out, pos, run, cleared, pmin, n == 0 ? 0 : lowest, price_taker, lmp);
#pragma unroll
  for (int i = 0; i < SP; ++i) {
    const bool first = keys[i] != kBidDrop && (i == 0 || bid_key_power(keys[i]) != bid_key_power(keys[i ? i - 1 : 0]));
    if (first) loop_emit_point(out, pos, run, cleared, bid_key_power(keys[i]), bid_key_price(keys[i]), price_taker, lmp);
  }
  *count = pos;
  return loop_curve_close(out, pos, S + 1, cleared);
}

}  // namespace dsp
