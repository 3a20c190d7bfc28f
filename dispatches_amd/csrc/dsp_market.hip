// dsp_market.hip — the stochastic mode of the wind + battery double loop on the device, gfx950 only (include/dsp_hip.h: dsp_market_*).
//
// Reference behaviour (run_double_loop_battery.py:81-105, 230-250): a Backcaster hands the Bidder n_scenario price scenarios taken
// from the last days' realised prices, the Bidder solves one LP per scenario and assembles a (power, marginal price) curve per hour
// (idaes Bidder._assemble_bids), the market dispatches the plant along that curve at the price that occurs.  Here for B plants at
// once; the S rows of plant b are rows b * S + i of the bidding LPs' batches.
//
//   market_prepare_kernel   scenario fan-out, one lane per row: objective entries, day-ahead power bounds, wind availability, realised
//                           state and objective constant of the row, prices gathered by the Backcaster's index rule (no stored
//                           history: in the price-taker setting the realised prices ARE the series).
//   market_clear_kernel     curve + clearing, one lane per (plant, period): the <= 16 composite keys of the lane (dsp_bid_cents.hpp)
//                           sit in registers and are sorted by a fully unrolled bitonic compare-exchange network (static register
//                           indices only: no LDS, no scratch - 0 bytes of scratch for every instantiation, checked with
//                           -Rpass-analysis=kernel-resource-usage); duplicates, the zero-power point and the running maximum are one
//                           pass over the sorted registers, which also clears the curve at the price that occurs.
//
//   loop_schedule_prepare_kernel   the coupled day-ahead LP of a self-scheduling plant (dsp_loop_schedule_prepare): S scenario blocks in
//                           ONE row per plant, one lane per (plant, scenario), the row's constant summed in the order of i by one lane
//                           (lmk_coupled_block).  A block is written once, by lmk_write_block, for every prepare kernel of the loop.
//   loop_monotone_prepare_kernel   the coupled day-ahead LP of a plant whose bid curve is monotone across its scenarios
//                           (dsp_loop_monotone_prepare, idaes' Bidder): the same blocks through the same lmk_coupled_block, and the
//                           bounds of the S (S - 1) / 2 * T ordered-pair rows from the order of the day-ahead scenario prices, one lane
//                           per (plant, pair, period).  The clearing reads such a row with dsp_loop_market_state::coupled = 1.
//   loop_midnight_prepare_kernel   the coupled REAL-TIME LP of the last T - 1 hours of a day (dsp_loop_midnight_prepare): the blocks of hour
//                           k through the same lmk_coupled_block, the pair rows' bounds from the order of the real-time scenario prices.
//   loop_market_prepare_kernel / loop_market_clear_kernel   the same two for ANY flowsheet, by descriptor (dsp_loop_market_*; rolling_flowsheets.py):
//                           power P_T = (x[a] ca + x[b] cb) + const, curves that start at the generator's p_min, <= 2 state columns,
//                           optional wind; the clearing lanes also write the tracker's LP (a dsp_loop_model).  VGPRs / scratch of every
//                           instantiation: profiles/loop_device_kernel_resources.txt.
//
// What the clearing kernels share with each other and with dsp_param.hip / dsp_project.hip lives in dsp_loop_device.hpp: the register
// barrier, the scenario index, sorted keys -> curve and cleared dispatch (loop_curve_and_clear, the wind + battery curve with
// p_min = 0), the wind window with its objective constant, and the plant half of the descriptor tracker's LP (loop_tracker_plant).
// Every product is made opaque before it is added: the results are bit-identical to the tensor operations of
// dispatches_amd/rolling.py / rolling_flowsheets.py (use_fused=False), which is how the kernels are tested.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dsp_hip.h"
#include "dsp_device.hpp"
#include "dsp_loop_device.hpp"

namespace dsp {

__global__ void __launch_bounds__(256) market_prepare_kernel(dsp_market_state s, dsp_market_model m, int k) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= s.B * s.S) return;
  const int b = r / s.S, i = r - b * s.S;
  const long long h = *s.hour, st0 = s.start[b];
  const int hod = k < 0 ? 0 : k;
  const int known = k < 0 ? 0 : min(m.T, 24 - k);
  double *c = m.c + (size_t)r * m.n, *lb = m.lb + (size_t)r * m.n, *ub = m.ub + (size_t)r * m.n;
  double avail_sum = 0.0;
  for (int t = 0; t < m.T; ++t) {
    const double rtp = s.rt_series[loop_scenario_index(s, st0, h, i, hod, t)];
    const double dap = t < known ? s.da_prices[(size_t)b * 24 + k + t] : s.da_series[loop_scenario_index(s, st0, h, i, hod, t)];
    const double r3 = loop_opaque(__dmul_rn(1e-3, rtp));
    c[m.pt_cols[t][0]] = __dsub_rn(m.base_c[m.pt_cols[t][0]], r3);
    c[m.pt_cols[t][1]] = __dsub_rn(m.base_c[m.pt_cols[t][1]], r3);
    c[m.pda_cols[t]] = __dsub_rn(m.base_c[m.pda_cols[t]], loop_opaque(__dsub_rn(dap, rtp)));
    const double avail = loop_opaque(__dmul_rn(m.wind_kw, s.cf_series[(st0 + h + t) % s.N]));      // capacity factors: the realised window
    ub[m.wind_cols[t]] = avail;
    avail_sum = t ? __dadd_rn(avail_sum, avail) : avail;
    const double fix = t < known ? s.da_offer[(size_t)b * 24 + k + t] : 0.0;
    lb[m.pda_cols[t]] = fix;
    ub[m.pda_cols[t]] = t < known ? fix : INFINITY;
  }
  if (m.c0) m.c0[r] = __dadd_rn(m.c0_base, loop_opaque(__dmul_rn(m.waste_per_kw, avail_sum)));
  const double soc = s.soc[b], thr = s.thr[b];
  lb[m.soc_init] = soc; ub[m.soc_init] = soc;
  lb[m.thr_init] = thr; ub[m.thr_init] = thr;
}

// bitonic network over SP keys in registers, ascending (every index a compile-time constant after unrolling); shared by both clearing kernels
template <int SP>
__device__ __forceinline__ void mk_sort(long long (&keys)[SP]) {
#pragma unroll
  for (int kk = 2; kk <= SP; kk <<= 1) {
#pragma unroll
    for (int j = kk >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < SP; ++i) {
        const int l = i ^ j;
        if (l > i) {
          const long long a = keys[i], c = keys[l];
          const bool swap = (a > c) == ((i & kk) == 0);
          keys[i] = swap ? c : a;
          keys[l] = swap ? a : c;
        }
      }
    }
  }
}

template <int SP>
__global__ void __launch_bounds__(256) market_clear_kernel(dsp_market_state s, dsp_market_model m, dsp_wb_model tr, int has_tr, int k, int T,
                                                           double *dispatch, int32_t *curve, int32_t *count) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= s.B * T) return;
  const int b = g / T, t = g - b * T;
  const int S = s.S;
  const long long h = *s.hour, st0 = s.start[b];
  const int hod = k < 0 ? 0 : k;
  const double *series = k < 0 ? s.da_series : s.rt_series;
  const int ca = k < 0 ? m.pda_cols[t] : m.pt_cols[t][0], cb = m.pt_cols[t][1];
  // ---- the S pairs of this plant and period as sort keys, in registers ----
  long long keys[SP];
  bool any_bad = false;
#pragma unroll
  for (int i = 0; i < SP; ++i) {
    long long key = kBidDrop;
    if (i < S) {
      const size_t row = (size_t)b * S + i;
      if (m.status[row] == 0) {
        const double *x = m.x + row * m.n;
        const double power = k < 0 ? x[ca] : __dmul_rn(1e-3, loop_opaque(__dadd_rn(x[ca], x[cb])));
        const double price = series[loop_scenario_index(s, st0, h, i, hod, t)];
        const long long pc = bid_cents(power), cc = bid_cents(price);
        if (pc >= 0 && fabs(power) < INFINITY && fabs(price) < INFINITY) key = bid_key(pc, cc);
      } else {
        any_bad = true;
      }
      if (t == 0 && m.flags && s.uncertified && (m.flags[row] & DSP_FLAG_OBJ_WAIVED))
        atomicAdd(reinterpret_cast<unsigned long long *>(s.uncertified), 1ull);
    }
    keys[i] = key;
  }
  if (any_bad && s.bad) *s.bad = 1;
  mk_sort<SP>(keys);
  // ---- the price that occurs: realised for the day-ahead market and for the hour at hand, scenario 0's for the look-ahead hours ----
  const double lmp = (k < 0 || t == 0) ? series[(st0 + h + t) % s.N] : series[loop_scenario_index(s, st0, h, 0, hod, t)];
  // ---- the curve from the zero-power point on, cleared at that price ----
  const double disp = loop_curve_and_clear<SP>(keys, S, 0, s.price_taker != 0, lmp, curve + (size_t)g * (S + 1) * 2, count + g);
  dispatch[g] = disp;
  if (k < 0) {
    s.da_prices[(size_t)b * 24 + t] = lmp;
    return;
  }
  if (!has_tr) return;
  // ---- the tracker's LP of this hour on the cleared dispatch ----
  double *rlo = tr.rlo + (size_t)b * tr.m, *rhi = tr.rhi + (size_t)b * tr.m;
  rlo[tr.track_rows[t]] = disp;
  rhi[tr.track_rows[t]] = disp;
  if (t == 0) {
    double *lb = tr.lb + (size_t)b * tr.n, *ub = tr.ub + (size_t)b * tr.n;
    const double avail_sum = loop_wind_window(ub, tr.wind_cols, tr.T, tr.wind_kw, s.cf_series, st0 + h, s.N);
    if (tr.c0) tr.c0[b] = loop_c0(tr.c0_base, tr.waste_per_kw, avail_sum);
    const double soc = s.soc[b], thr = s.thr[b];
    lb[tr.soc_init] = soc; ub[tr.soc_init] = soc;
    lb[tr.thr_init] = thr; ub[tr.thr_init] = thr;
  }
}

hipError_t launch_market_prepare(const dsp_market_state &st, const dsp_market_model &m, int k, hipStream_t stream) {
  const long long rows = (long long)st.B * st.S;
  hipLaunchKernelGGL(market_prepare_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, st, m, k);
  return hipGetLastError();
}

hipError_t launch_market_clear(const dsp_market_state &st, const dsp_market_model &m, const dsp_wb_model *tr, int k, int T, double *dispatch,
                               int32_t *curve, int32_t *count, hipStream_t stream) {
  const long long lanes = (long long)st.B * T;
  const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
  const dsp_wb_model trv = tr ? *tr : dsp_wb_model{};
  const int has_tr = tr != nullptr;
#define DSP_MK_LAUNCH(SP) hipLaunchKernelGGL(market_clear_kernel<SP>, grid, block, 0, stream, st, m, trv, has_tr, k, T, dispatch, curve, count)
  if (st.S <= 1) DSP_MK_LAUNCH(1);
  else if (st.S <= 2) DSP_MK_LAUNCH(2);
  else if (st.S <= 4) DSP_MK_LAUNCH(4);
  else if (st.S <= 8) DSP_MK_LAUNCH(8);
  else DSP_MK_LAUNCH(16);
#undef DSP_MK_LAUNCH
  return hipGetLastError();
}

// ---- the same two kernels for a flowsheet given by a descriptor (include/dsp_hip.h: dsp_loop_market_*; rolling_flowsheets.py) ----------
// Bit-identical to BatchedDoubleLoop's tensor form (use_fused=False): every product opaque before it is added, sums in the order of t.
static_assert(sizeof(dsp_loop_market_state) + sizeof(dsp_loop_market_model) + sizeof(dsp_loop_model) + 64 <= 4096,
              "the descriptors travel as by-value kernel arguments: HIP's limit is 4 KB");

// the same hour of the REAL-TIME series: with the backcast forecaster its history ends rt_history_lag_days earlier (ABI 17; a bid made
// at the RUC hour: today is not a whole day of real-time prices yet).  lag 0: `at` itself.  24 * lag < N is checked on the host.
__device__ __forceinline__ long long lmk_rt(const dsp_loop_market_state &s, long long at) {
  if (!s.backcast || s.rt_history_lag_days == 0) return at;
  const long long v = at - 24ll * s.rt_history_lag_days;
  return v < 0 ? v + s.N : v;
}

// sum_t rt[t] pt_const[t] of scenario j's real-time prices asked at hour-of-day hod, in the order of t: the prices' share of a block's
// objective constant
__device__ __forceinline__ double lmk_price_sum(const dsp_loop_market_state &s, const dsp_loop_market_model &m, long long st0, long long h,
                                                int j, int hod) {
  double price_sum = 0.0;
  for (int t = 0; t < m.T; ++t) {
    const double rtp = s.rt_series[lmk_rt(s, loop_scenario_index(s, st0, h, j, hod, t))];
    const double pc = loop_opaque(__dmul_rn(rtp, m.pt_const[t]));
    price_sum = t ? __dadd_rn(price_sum, pc) : pc;
  }
  return price_sum;
}

// One bidding block - c / lb / ub of a row of a bidding batch, or of scenario block i of a coupled row - of plant b at hour k of the
// day (-1: the day-ahead bid): objective entries of the two power terms and of day_ahead_power on scenario i's prices, wind bounds of
// the realised window (wind size kw), day_ahead_power fixed to the cleared offer inside the cleared day and free beyond it, state
// columns.  Returns what the block's objective constant takes: sum_t rt[t] pt_const[t] and sum_t avail[t], each in the order of t.
struct lmk_sums { double price, avail; };
__device__ __forceinline__ lmk_sums lmk_write_block(const dsp_loop_market_state &s, const dsp_loop_market_model &m, double *c, double *lb,
                                                    double *ub, int b, int i, int k, double kw) {
  const long long h = *s.hour, st0 = s.start[b];
  const int hod = k < 0 ? 0 : k;
  const int known = k < 0 ? 0 : min(m.T, 24 - k);
  const bool wind = m.wind_cols[0] >= 0;
  double avail_sum = 0.0, price_sum = 0.0;
  for (int t = 0; t < m.T; ++t) {
    const long long at = loop_scenario_index(s, st0, h, i, hod, t);
    const double rtp = s.rt_series[lmk_rt(s, at)];
    const double dap = t < known ? s.da_prices[(size_t)b * 24 + k + t] : s.da_series[at];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int col = m.pt_cols[t][e];
      if (col >= 0) c[col] = __dsub_rn(m.base_c[col], loop_opaque(__dmul_rn(m.pt_coef[t][e], rtp)));
    }
    const int pda = m.pda_cols[t];
    c[pda] = __dsub_rn(m.base_c[pda], loop_opaque(__dsub_rn(dap, rtp)));
    const double pc = loop_opaque(__dmul_rn(rtp, m.pt_const[t]));
    price_sum = t ? __dadd_rn(price_sum, pc) : pc;
    if (wind) {
      const double avail = loop_opaque(__dmul_rn(kw, s.cf_series[(st0 + h + t) % s.N]));     // capacity factors: the realised window
      ub[m.wind_cols[t]] = avail;
      avail_sum = t ? __dadd_rn(avail_sum, avail) : avail;
    }
    const double fix = t < known ? s.da_offer[(size_t)b * 24 + k + t] : 0.0;
    lb[pda] = fix;
    ub[pda] = t < known ? fix : INFINITY;
  }
  for (int j = 0; j < m.n_state; ++j) {
    const double v = s.state[(size_t)b * m.n_state + j];
    lb[m.state_init[j]] = v; ub[m.state_init[j]] = v;
  }
  return {price_sum, avail_sum};
}

// a block's objective constant: (base - price_sum) + waste, the wind term only where there is wind
__device__ __forceinline__ double lmk_c0(double base, double price_sum, bool wind, double waste) {
  const double c0 = loop_opaque(__dsub_rn(base, price_sum));
  return wind ? loop_opaque(__dadd_rn(c0, waste)) : c0;
}

__global__ void __launch_bounds__(256) loop_market_prepare_kernel(dsp_loop_market_state s, dsp_loop_market_model m, int k) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= s.B * s.S) return;
  const int b = r / s.S, i = r - b * s.S;
  const bool wind = m.wind_cols[0] >= 0;
  const double kw = m.wind_kw_plant ? m.wind_kw_plant[b] : m.wind_kw;       // per-plant sizes (ABI 16): row r belongs to plant b = r / S
  const double c0_base = m.c0_base_plant ? m.c0_base_plant[b] : m.c0_base;
  const size_t at0 = (size_t)r * m.n;
  const lmk_sums sums = lmk_write_block(s, m, m.c + at0, m.lb + at0, m.ub + at0, b, i, k, kw);
  m.c0[r] = lmk_c0(c0_base, sums.price, wind, wind ? loop_opaque(__dmul_rn(m.waste_per_kw, sums.avail)) : 0.0);
}

// Lane r = b * S + i of a coupled day-ahead LP: S scenario blocks of m.n columns side by side in row b (m.row_stride doubles apart).
// Block i is the block that loop_market_prepare_kernel writes into row b * S + i at hour k of the day (-1: the day-ahead bid); the lane
// of scenario 0 also sums the S objective constants in the order of i - alone, so that the order is the tensor form's
// (BatchedDoubleLoop._coupled_blocks / _tied_blocks).  One block writer and one constant summer for the self-schedule's rows and the
// monotone Bidder's, day-ahead and - the look-ahead hours past midnight - real-time.
__device__ __forceinline__ void lmk_coupled_block(const dsp_loop_market_state &s, const dsp_loop_market_model &m, int r, int k) {
  const int b = r / s.S, i = r - b * s.S;
  const bool wind = m.wind_cols[0] >= 0;
  const size_t at0 = (size_t)b * m.row_stride + (size_t)i * m.n;
  const lmk_sums sums = lmk_write_block(s, m, m.c + at0, m.lb + at0, m.ub + at0, b, i, k, m.wind_kw);
  if (i != 0) return;
  // ---- the row's objective constant: the S scenario constants added in the order of i ----
  const long long h = *s.hour, st0 = s.start[b];
  const double waste = wind ? loop_opaque(__dmul_rn(m.waste_per_kw, sums.avail)) : 0.0;
  double total = 0.0;
  for (int j = 0; j < s.S; ++j) {
    const double c0 = lmk_c0(m.c0_base, lmk_price_sum(s, m, st0, h, j, k < 0 ? 0 : k), wind, waste);
    total = j ? __dadd_rn(total, c0) : c0;
  }
  m.c0[b] = total;
}

// The coupled day-ahead LP of a self-scheduling plant (dsp_loop_schedule_prepare, ABI 18): one lane per (plant, scenario); its coupling
// rows are static (bounds 0, 0, written once by the caller).
__global__ void __launch_bounds__(256) loop_schedule_prepare_kernel(dsp_loop_market_state s, dsp_loop_market_model m) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= s.B * s.S) return;
  lmk_coupled_block(s, m, r, -1);
}

// The coupled day-ahead LP of a plant that bids a MONOTONE curve (dsp_loop_monotone_prepare, ABI 19; idaes' Bidder): the same S blocks,
// tied by P = S (S - 1) / 2 rows pda[k, t] - pda[j, t] per period (pairs j < k, k fastest; row first + p * T + t) whose BOUNDS follow
// the order of plant b's day-ahead scenario prices: with d = da[k, t] - da[j, t], rlo = 0 if d > 0 else -inf, rhi = 0 if d < 0 else +inf
// (CoupledScenarioModel.load).  One launch over two lane ranges: lanes [0, B * S) write the blocks and the constant as above, the next
// B * P * T lanes one (b, p, t) each, t fastest - a wave's stores to a row of rlo / rhi are consecutive.  No atomics, no cross-lane
// traffic; every lane writes addresses of its own.
__global__ void __launch_bounds__(256) loop_monotone_prepare_kernel(dsp_loop_market_state s, dsp_loop_market_model m, double *rlo, double *rhi,
                                                                    int m_rows, int first) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int S = s.S, T = m.T;
  const long long blocks = (long long)s.B * S;
  if (g < blocks) {
    lmk_coupled_block(s, m, (int)g, -1);
    return;
  }
  const int per_plant = S * (S - 1) / 2 * T;
  const long long q = g - blocks;
  if (q >= (long long)s.B * per_plant) return;
  const int b = (int)(q / per_plant), pt = (int)(q - (long long)b * per_plant);
  const int p = pt / T, t = pt - p * T;
  int j = 0, rest = p;                           // p -> (j, k): pairs (0, 1) .. (0, S - 1), (1, 2) ..: at most 15 values of j
  while (rest >= S - 1 - j) { rest -= S - 1 - j; ++j; }
  const int k = j + 1 + rest;
  const long long h = *s.hour, st0 = s.start[b];
  const double d = __dsub_rn(s.da_series[loop_scenario_index(s, st0, h, k, 0, t)], s.da_series[loop_scenario_index(s, st0, h, j, 0, t)]);
  const size_t at = (size_t)b * m_rows + first + pt;
  rlo[at] = d > 0.0 ? 0.0 : -INFINITY;
  rhi[at] = d < 0.0 ? 0.0 : INFINITY;
}

// The coupled REAL-TIME LP of hour k of the day, in the last T - 1 hours of a day (dsp_loop_midnight_prepare; BatchedDoubleLoop with
// past_midnight="coupled"): the S blocks of row b are the rows b * S + i that loop_market_prepare_kernel writes at hour k - day_ahead_power
// fixed to the cleared offer inside the day, free past midnight - and c0[b] their constants summed in the order of i.  The monotone
// Bidder's pair rows cover ALL T periods and follow the order of the hour's REAL-TIME scenario prices (the backcast asked at hour-of-day
// k, through lmk_rt): one lane per (b, pair, t), t fastest, exactly loop_monotone_prepare_kernel's second lane range.  rlo == NULL: a
// self-schedule, whose coupling rows are static.  No atomics, no cross-lane traffic; every lane writes addresses of its own.
__global__ void __launch_bounds__(256) loop_midnight_prepare_kernel(dsp_loop_market_state s, dsp_loop_market_model m, double *rlo, double *rhi,
                                                                    int m_rows, int first, int k) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int S = s.S, T = m.T;
  const long long blocks = (long long)s.B * S;
  if (g < blocks) {
    lmk_coupled_block(s, m, (int)g, k);
    return;
  }
  if (!rlo) return;
  const int per_plant = S * (S - 1) / 2 * T;
  const long long q = g - blocks;
  if (q >= (long long)s.B * per_plant) return;
  const int b = (int)(q / per_plant), pt = (int)(q - (long long)b * per_plant);
  const int p = pt / T, t = pt - p * T;
  int j = 0, rest = p;                           // p -> (j, kk): pairs (0, 1) .. (0, S - 1), (1, 2) ..: at most 15 values of j
  while (rest >= S - 1 - j) { rest -= S - 1 - j; ++j; }
  const int kk = j + 1 + rest;
  const long long h = *s.hour, st0 = s.start[b];
  const double d = __dsub_rn(s.rt_series[lmk_rt(s, loop_scenario_index(s, st0, h, kk, k, t))],
                             s.rt_series[lmk_rt(s, loop_scenario_index(s, st0, h, j, k, t))]);
  const size_t at = (size_t)b * m_rows + first + pt;
  rlo[at] = d > 0.0 ? 0.0 : -INFINITY;
  rhi[at] = d < 0.0 ? 0.0 : INFINITY;
}

template <int SP>
__global__ void __launch_bounds__(256) loop_market_clear_kernel(dsp_loop_market_state s, dsp_loop_market_model m, dsp_loop_model tr, int has_tr,
                                                                int k, int T, double *dispatch, int32_t *curve, int32_t *count) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= s.B * T) return;
  const int b = g / T, t = g - b * T;
  const int S = s.S;
  const long long h = *s.hour, st0 = s.start[b];
  const long long pmin = s.p_min_cents_plant ? s.p_min_cents_plant[b] : s.p_min_cents;      // (ABI 20: per plant at the site of the scalar)
  const int hod = k < 0 ? 0 : k;
  const double *series = k < 0 ? s.da_series : s.rt_series;
  const int ca = k < 0 ? m.pda_cols[t] : m.pt_cols[t][0], cb = k < 0 ? -1 : m.pt_cols[t][1];
  const double fa = m.pt_coef[t][0], fb = m.pt_coef[t][1], fc = m.pt_const[t];
  // ---- the S pairs of this plant and period as sort keys, in registers ----
  long long keys[SP];
  bool any_bad = false;
#pragma unroll
  for (int i = 0; i < SP; ++i) {
    long long key = kBidDrop;
    if (i < S) {
      // (ABI 19, coupled: scenario i of plant b is block i of row b, one status / flags entry per plant; ABI 18: block 0 of a coupled row)
      const size_t row = s.coupled ? (size_t)b : (size_t)b * S + i;
      if (m.status[row] == 0) {
        const double *x = m.x + row * (size_t)(m.row_stride ? m.row_stride : m.n) + (s.coupled ? (size_t)i * m.n : 0);
        double power;
        if (k < 0) {
          power = x[ca];
        } else {
          double p = ca >= 0 ? loop_opaque(__dmul_rn(x[ca], fa)) : 0.0;
          if (cb >= 0) p = loop_opaque(__dadd_rn(p, loop_opaque(__dmul_rn(x[cb], fb))));
          power = __dadd_rn(p, fc);
        }
        const long long at = loop_scenario_index(s, st0, h, i, hod, t);
        const double price = s.self_schedule ? 0.0 : series[k < 0 ? at : lmk_rt(s, at)];      // (ABI 18: a schedule is offered at cost 0)
        const long long pc = bid_cents(power), cc = bid_cents(price);
        if (pc >= pmin && fabs(power) < INFINITY && fabs(price) < INFINITY) key = bid_key(pc, cc);
      } else {
        any_bad = true;
      }
      if (t == 0 && (i == 0 || !s.coupled) && m.flags && s.uncertified && (m.flags[row] & DSP_FLAG_OBJ_WAIVED))      // (coupled: a plant once)
        atomicAdd(reinterpret_cast<unsigned long long *>(s.uncertified), 1ull);
    }
    keys[i] = key;
  }
  if (any_bad && s.bad) *s.bad = 1;
  mk_sort<SP>(keys);
  // ---- the price that occurs: realised for the day-ahead market and for the hour at hand, scenario 0's for the look-ahead hours ----
  const double lmp = (k < 0 || t == 0) ? series[(st0 + h + t) % s.N] : series[lmk_rt(s, loop_scenario_index(s, st0, h, 0, hod, t))];
  // ---- the curve from the p_min point on, cleared at that price ----
  const int slots = s.curve_slots ? s.curve_slots : S + 1;      // (ABI 18: points per stored curve)
  const double disp = loop_curve_and_clear<SP>(keys, slots - 1, pmin, s.price_taker != 0, lmp, curve + (size_t)g * slots * 2, count + g);
  dispatch[g] = disp;
  if (k < 0) {
    s.da_prices[(size_t)b * 24 + t] = lmp;
    return;
  }
  if (!has_tr) return;
  // ---- the tracker's LP of this hour on the cleared dispatch ----
  double *rlo = tr.rlo + (size_t)b * tr.m, *rhi = tr.rhi + (size_t)b * tr.m;
  const double rhs = __dsub_rn(disp, tr.pt_const[t]);
  rlo[tr.track_rows[t]] = rhs;
  rhi[tr.track_rows[t]] = rhs;
  if (t == 0) loop_tracker_plant(tr, b, s.cf_series, st0 + h, s.N, s.state + (size_t)b * tr.n_state);
}

hipError_t launch_loop_market_prepare(const dsp_loop_market_state &st, const dsp_loop_market_model &m, int k, hipStream_t stream) {
  const long long rows = (long long)st.B * st.S;
  hipLaunchKernelGGL(loop_market_prepare_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, st, m, k);
  return hipGetLastError();
}

hipError_t launch_loop_schedule_prepare(const dsp_loop_market_state &st, const dsp_loop_market_model &m, hipStream_t stream) {
  const long long rows = (long long)st.B * st.S;
  hipLaunchKernelGGL(loop_schedule_prepare_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, st, m);
  return hipGetLastError();
}

hipError_t launch_loop_monotone_prepare(const dsp_loop_market_state &st, const dsp_loop_market_model &m, double *rlo, double *rhi, int m_rows,
                                        int first, hipStream_t stream) {
  const long long lanes = (long long)st.B * st.S + (long long)st.B * (st.S * (st.S - 1) / 2) * m.T;
  hipLaunchKernelGGL(loop_monotone_prepare_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, st, m, rlo, rhi, m_rows, first);
  return hipGetLastError();
}

hipError_t launch_loop_midnight_prepare(const dsp_loop_market_state &st, const dsp_loop_market_model &m, double *rlo, double *rhi, int m_rows,
                                        int first, int k, hipStream_t stream) {
  const long long lanes = (long long)st.B * st.S + (rlo ? (long long)st.B * (st.S * (st.S - 1) / 2) * m.T : 0);
  hipLaunchKernelGGL(loop_midnight_prepare_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, st, m, rlo, rhi, m_rows, first, k);
  return hipGetLastError();
}

hipError_t launch_loop_market_clear(const dsp_loop_market_state &st, const dsp_loop_market_model &m, const dsp_loop_model *tr, int k, int T,
                                    double *dispatch, int32_t *curve, int32_t *count, hipStream_t stream) {
  const long long lanes = (long long)st.B * T;
  const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
  const dsp_loop_model trv = tr ? *tr : dsp_loop_model{};
  const int has_tr = tr != nullptr;
#define DSP_LMK_LAUNCH(SP) hipLaunchKernelGGL(loop_market_clear_kernel<SP>, grid, block, 0, stream, st, m, trv, has_tr, k, T, dispatch, curve, count)
  if (st.S <= 1) DSP_LMK_LAUNCH(1);
  else if (st.S <= 2) DSP_LMK_LAUNCH(2);
  else if (st.S <= 4) DSP_LMK_LAUNCH(4);
  else if (st.S <= 8) DSP_LMK_LAUNCH(8);
  else DSP_LMK_LAUNCH(16);
#undef DSP_LMK_LAUNCH
  return hipGetLastError();
}

}  // namespace dsp
