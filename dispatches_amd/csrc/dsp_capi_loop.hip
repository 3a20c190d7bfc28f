// dsp_capi_loop.hip — the C ABI of the double loops, the bid kernel and the market kernels: descriptors checked on the host, then one launch_*
#include <cmath>
#include <vector>

#include "dsp_capi_internal.hpp"
#include "dsp_record_check.hpp"

using namespace dsp;

// ---- descriptors checked on the host: every index a lane would use lies inside its buffer, nothing is launched otherwise ----
static bool market_col_ok(int32_t col, int32_t n) { return col >= 0 && col < n; }
static bool loop_cols_ok(const int32_t *cols, int count, int32_t n) {
  for (int i = 0; i < count; ++i)
    if (!market_col_ok(cols[i], n)) return false;
  return true;
}
// the <= 2 terms of the power output of T periods: a column of the LP, or -1 for "no such term"
static bool loop_terms_ok(const int32_t (*pt_cols)[2], int T, int32_t n) {
  for (int t = 0; t < T; ++t)
    for (int e = 0; e < 2; ++e)
      if (pt_cols[t][e] != -1 && !market_col_ok(pt_cols[t][e], n)) return false;
  return true;
}
// wind columns of T periods (none: wind_cols[0] < 0) need the capacity factors
static bool loop_wind_ok(const int32_t *wind_cols, int T, int32_t n, const void *cf_series) {
  return wind_cols[0] < 0 || (cf_series && loop_cols_ok(wind_cols, T, n));
}
// per-plant sizes (ABI 16): both pointers or neither, and only on a model that has wind columns
static bool plant_sizes_ok(const double *wind_kw_plant, const double *c0_base_plant, int32_t wind_col0) {
  if (!wind_kw_plant != !c0_base_plant) return false;
  return !wind_kw_plant || wind_col0 >= 0;
}
// the indices of a tracker of horizon T whose dispatch rows and plant half (loop_tracker_plant) a kernel writes
static bool loop_tracker_cols_ok(const dsp_loop_model *tr, int T, const void *state, const void *cf_series) {
  if (tr->n_state < 0 || tr->n_state > 2 || (tr->n_state > 0 && !state)) return false;
  return loop_cols_ok(tr->state_init, tr->n_state, tr->n) && loop_cols_ok(tr->track_rows, T, tr->m) && loop_wind_ok(tr->wind_cols, T, tr->n, cf_series) &&
         plant_sizes_ok(tr->wind_kw_plant, tr->c0_base_plant, tr->wind_cols[0]);
}
// ... and its buffers: safe to launch a kernel that writes the tracker's LP
static bool loop_tracker_ok(const dsp_loop_model *tr, int T, const void *state, const void *cf_series) {
  if (!tr || T < 1 || T > DSP_LOOP_MAX_T || tr->T != T || tr->n < 1 || tr->m < 1) return false;
  if (!tr->lb || !tr->ub || !tr->rlo || !tr->rhi || !tr->c0) return false;
  return loop_tracker_cols_ok(tr, T, state, cf_series);
}
// arguments of the stochastic mode's entry points, checked on the host: nothing is launched on a bad descriptor
static bool market_state_ok(const dsp_market_state *st) {
  if (!st || st->B < 0 || st->N < 1 || st->S < 1 || st->S > DSP_MARKET_MAX_S) return false;
  if (st->backcast ? (st->D < 1 || st->S > st->D || 24ll * st->D > st->N) : st->S != 1) return false;
  return st->start && st->hour && st->da_series && st->rt_series;
}
// ... and of the descriptor loop's (dsp_loop_market_*): every index a kernel would use is checked here, nothing is launched otherwise
static bool loop_market_state_ok(const dsp_loop_market_state *st) {
  if (!st || st->B < 0 || st->N < 1 || st->S < 1 || st->S > DSP_MARKET_MAX_S || st->p_min_cents < 0 || st->p_min_cents > 2000000000ll) return false;
  if (st->backcast ? (st->D < 1 || st->S > st->D || 24ll * st->D > st->N) : st->S != 1) return false;
  if (st->rt_history_lag_days < 0 || (st->backcast && 24ll * ((long long)st->D + st->rt_history_lag_days) > st->N)) return false;      // (ABI 17)
  if (st->self_schedule < 0 || st->self_schedule > 1) return false;                                                                     // (ABI 18)
  if (st->curve_slots != 0 && (st->curve_slots < st->S + 1 || st->curve_slots > DSP_MARKET_MAX_S + 1)) return false;
  if (st->coupled < 0 || st->coupled > 1 || (st->coupled && st->self_schedule)) return false;                                           // (ABI 19)
  return st->start && st->hour && st->da_series && st->rt_series;
}
static bool loop_market_model_ok(const dsp_loop_market_model *m) {
  return m && m->n >= 1 && m->T >= 1 && m->T <= DSP_MARKET_MAX_T && m->n_state >= 0 && m->n_state <= 2 &&
         (m->row_stride == 0 || m->row_stride >= m->n);                                                                                 // (ABI 18)
}
// the checks dsp_loop_market_prepare and dsp_loop_schedule_prepare share: every buffer and column index a lane writes through
static bool loop_market_prepare_ok(const dsp_loop_market_state *st, const dsp_loop_market_model *m) {
  if (!m->c || !m->lb || !m->ub || !m->base_c || !m->c0) return false;
  if ((m->n_state > 0 && !st->state) || !loop_cols_ok(m->state_init, m->n_state, m->n)) return false;
  if (!loop_wind_ok(m->wind_cols, m->T, m->n, st->cf_series) || !plant_sizes_ok(m->wind_kw_plant, m->c0_base_plant, m->wind_cols[0])) return false;
  return loop_cols_ok(m->pda_cols, m->T, m->n) && loop_terms_ok(m->pt_cols, m->T, m->n);
}

// per-plant minimum powers (ABI 20): a device array, read back and bounded like the scalar - except on a capturing stream, which
// cannot be read on (the loops run their first day eagerly)
static bool plant_p_min_ok(const dsp_loop_market_state *st, hipStream_t stream) {
  if (!st->p_min_cents_plant || st->B == 0) return true;
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &capturing) != hipSuccess) return false;
  if (capturing != hipStreamCaptureStatusNone) return true;
  std::vector<int64_t> host((size_t)st->B);
  if (hipMemcpyAsync(host.data(), st->p_min_cents_plant, host.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) != hipSuccess) return false;
  if (hipStreamSynchronize(stream) != hipSuccess) return false;
  for (int64_t v : host)
    if (v < 0 || v > 2000000000ll) return false;
  return true;
}

extern "C" {

int dsp_wb_rolling_update(const dsp_wb_state *st, const dsp_wb_model *rt, const dsp_wb_model *tr, int32_t phase, int32_t k, void *hipStream) {
  if (!st || !rt || !tr || st->B < 0 || phase < 0 || phase > 2 || k < 0 || k > 23 || rt->T < 1 || rt->T > 8 || tr->T < 1 || tr->T > 8)
    return DSP_ERR_INVALID;
  if (st->B == 0) return DSP_OK;
  HIP_TRY(launch_wb_rolling(*st, *rt, *tr, (int)phase, (int)k, (hipStream_t)hipStream));
  return DSP_OK;
}

int dsp_loop_update(const dsp_loop_state *st, const dsp_loop_model *rt, const dsp_loop_model *tr, int32_t phase, int32_t k, void *hipStream) {
  if (!st || !rt || !tr || st->B < 0 || phase < 0 || phase > 2 || k < 0 || k > 23 || rt->T < 1 || rt->T > DSP_LOOP_MAX_T || tr->T < 1 ||
      tr->T > DSP_LOOP_MAX_T || rt->n_state < 0 || rt->n_state > 2 || tr->n_state != rt->n_state || !rt->c0 || !tr->c0)
    return DSP_ERR_INVALID;
  // per-plant sizes (ABI 16): both pointers or neither on each model, the two models together, only with wind columns
  if (!plant_sizes_ok(rt->wind_kw_plant, rt->c0_base_plant, rt->wind_cols[0]) || !rt->wind_kw_plant != !tr->wind_kw_plant) return DSP_ERR_INVALID;
  // every index of the three phases.  The tracker follows the first tr->T periods of the real-time offer (phase 2 reads the tracker
  // alone: the parametrized mode, which has no real-time LP, calls it with tracking horizons beyond the real-time one)
  if ((phase < 2 && tr->T > rt->T) || !loop_tracker_cols_ok(tr, tr->T, st->state, st->cf_series) || !loop_cols_ok(tr->state_real, tr->n_state, tr->n) ||
      !loop_terms_ok(tr->pt_cols, tr->T, tr->n))
    return DSP_ERR_INVALID;
  if (!loop_cols_ok(rt->pda_cols, rt->T, rt->n) || !loop_terms_ok(rt->pt_cols, rt->T, rt->n) || !loop_cols_ok(rt->state_init, rt->n_state, rt->n) ||
      !loop_wind_ok(rt->wind_cols, rt->T, rt->n, st->cf_series))
    return DSP_ERR_INVALID;
  if (st->B == 0) return DSP_OK;
  HIP_TRY(launch_loop_update(*st, *rt, *tr, (int)phase, (int)k, (hipStream_t)hipStream));
  return DSP_OK;
}

// the ledger of the implemented hour (ABI 20): every index and pointer a lane would use is checked here
int dsp_loop_ledger(const dsp_loop_state *st, const dsp_loop_model *tr, const dsp_loop_ledger_desc *g, void *hipStream) {
  if (!st || !tr || !g || st->B < 0 || tr->n < 1 || !tr->x) return DSP_ERR_INVALID;
  if (g->n_forms < 1 || g->n_forms > DSP_LEDGER_MAX_FORMS || g->reserved != 0) return DSP_ERR_INVALID;
  if (!g->acc || !g->hour_value || !g->coef || !g->constant) return DSP_ERR_INVALID;
  if (g->coef_stride < 0 || (g->coef_stride != 0 && g->coef_stride < (int64_t)g->n_forms * DSP_LEDGER_MAX_TERMS)) return DSP_ERR_INVALID;
  if (g->const_stride < 0 || (g->const_stride != 0 && g->const_stride < g->n_forms)) return DSP_ERR_INVALID;
  for (int f = 0; f < g->n_forms; ++f) {
    if (g->n_terms[f] < 0 || g->n_terms[f] > DSP_LEDGER_MAX_TERMS || !loop_cols_ok(g->cols[f], g->n_terms[f], tr->n)) return DSP_ERR_INVALID;
    if (g->per_avail[f] == 0.0) continue;
    // the wind available in the hour: the tracker's wind size (per plant with both of its pointers, ABI 16), the series, the clock
    if (!std::isfinite(g->per_avail[f]) || tr->wind_cols[0] < 0 || !st->cf_series || !st->start || !st->hour || st->N < 1) return DSP_ERR_INVALID;
    if (!plant_sizes_ok(tr->wind_kw_plant, tr->c0_base_plant, tr->wind_cols[0])) return DSP_ERR_INVALID;
  }
  if (st->B == 0) return DSP_OK;
  HIP_TRY(launch_loop_ledger(*st, *tr, *g, (hipStream_t)hipStream));
  return DSP_OK;
}

// the recorder (ABI 21): the descriptor's check is dsp_record_check.hpp's, every plant index included
int dsp_loop_record(const dsp_loop_record_desc *rec, int32_t B, void *hipStream) {
  if (!loop_record_ok(rec, B)) return DSP_ERR_INVALID;
  HIP_TRY(launch_loop_record(*rec, (hipStream_t)hipStream));
  return DSP_OK;
}

int dsp_bid_points(const dsp_bid_request *rq, void *hipStream) {
  if (!rq || rq->B < 0 || rq->T < 0 || rq->terms < 0 || rq->terms > 2 || rq->ldx < 1 || rq->ldp < rq->T) return DSP_ERR_INVALID;
  if (rq->B > DSP_BID_MAX_SCENARIOS || rq->T > DSP_BID_MAX_HOURS) return DSP_ERR_TOO_LARGE;
  if (rq->T == 0) return DSP_OK;
  if (!rq->out || (rq->B > 0 && (!rq->x || !rq->price))) return DSP_ERR_INVALID;
  for (int t = 0; t < rq->T; ++t)
    for (int e = 0; e < (rq->terms == 2 ? 2 : 1); ++e)
      if (rq->col[t][e] < 0 || rq->col[t][e] >= rq->ldx) return DSP_ERR_INVALID;
  HIP_TRY(launch_bid_points(*rq, (hipStream_t)hipStream));
  return DSP_OK;
}

int dsp_market_prepare(const dsp_market_state *st, const dsp_market_model *m, int32_t k, void *hipStream) {
  if (!market_state_ok(st) || !m || k < -1 || k > 23 || m->n < 1 || m->T < 1 || m->T > DSP_MARKET_MAX_T) return DSP_ERR_INVALID;
  if (!st->cf_series || !st->soc || !st->thr || !m->c || !m->lb || !m->ub || !m->base_c) return DSP_ERR_INVALID;
  if (k >= 0 && (!st->da_offer || !st->da_prices)) return DSP_ERR_INVALID;
  if (!market_col_ok(m->soc_init, m->n) || !market_col_ok(m->thr_init, m->n)) return DSP_ERR_INVALID;
  for (int t = 0; t < m->T; ++t)
    if (!market_col_ok(m->wind_cols[t], m->n) || !market_col_ok(m->pt_cols[t][0], m->n) || !market_col_ok(m->pt_cols[t][1], m->n) ||
        !market_col_ok(m->pda_cols[t], m->n))
      return DSP_ERR_INVALID;
  if (st->B == 0) return DSP_OK;
  HIP_TRY(launch_market_prepare(*st, *m, (int)k, (hipStream_t)hipStream));
  return DSP_OK;
}

int dsp_market_clear(const dsp_market_state *st, const dsp_market_model *m, const dsp_wb_model *tr, int32_t k, int32_t T,
                     double *dispatch, int32_t *curve, int32_t *count, void *hipStream) {
  if (!market_state_ok(st) || !m || k < -1 || k > 23 || m->n < 1 || m->T < 1 || m->T > DSP_MARKET_MAX_T || T < 1 || T > m->T) return DSP_ERR_INVALID;
  if (!m->x || !m->status || !dispatch || !curve || !count) return DSP_ERR_INVALID;
  if (k < 0 ? (T > 24 || !st->da_prices || tr) : T > 8) return DSP_ERR_INVALID;
  for (int t = 0; t < T; ++t)
    if (k < 0 ? !market_col_ok(m->pda_cols[t], m->n) : (!market_col_ok(m->pt_cols[t][0], m->n) || !market_col_ok(m->pt_cols[t][1], m->n)))
      return DSP_ERR_INVALID;
  if (tr) {
    if (tr->T != T || tr->n < 1 || tr->m < 1 || !tr->lb || !tr->ub || !tr->rlo || !tr->rhi || !st->cf_series || !st->soc || !st->thr) return DSP_ERR_INVALID;
    if (!market_col_ok(tr->soc_init, tr->n) || !market_col_ok(tr->thr_init, tr->n)) return DSP_ERR_INVALID;
    for (int t = 0; t < T; ++t)
      if (!market_col_ok(tr->wind_cols[t], tr->n) || !market_col_ok(tr->track_rows[t], tr->m)) return DSP_ERR_INVALID;
  }
  if (st->B == 0) return DSP_OK;
  HIP_TRY(launch_market_clear(*st, *m, tr, (int)k, (int)T, dispatch, curve, count, (hipStream_t)hipStream));
  return DSP_OK;
}

int dsp_loop_market_prepare(const dsp_loop_market_state *st, const dsp_loop_market_model *m, int32_t k, void *hipStream) {
  if (!loop_market_state_ok(st) || !loop_market_model_ok(m) || k < -1 || k > 23) return DSP_ERR_INVALID;
  if (m->row_stride != 0 && m->row_stride != m->n) return DSP_ERR_INVALID;      // (ABI 18: its rows are n apart)
  if (k >= 0 && (!st->da_offer || !st->da_prices)) return DSP_ERR_INVALID;
  if (!loop_market_prepare_ok(st, m)) return DSP_ERR_INVALID;
  if (st->B == 0) return DSP_OK;
  HIP_TRY(launch_loop_market_prepare(*st, *m, (int)k, (hipStream_t)hipStream));
  return DSP_OK;
}

// the coupled day-ahead LP of a self-scheduling plant (ABI 18): `m` describes one of the S blocks of a row of row_stride doubles
int dsp_loop_schedule_prepare(const dsp_loop_market_state *st, const dsp_loop_market_model *m, void *hipStream) {
  if (!loop_market_state_ok(st) || !loop_market_model_ok(m)) return DSP_ERR_INVALID;
  if ((long long)m->row_stride < (long long)st->S * m->n) return DSP_ERR_INVALID;
  if (!loop_market_prepare_ok(st, m) || m->wind_kw_plant || m->c0_base_plant) return DSP_ERR_INVALID;
  if (st->B == 0) return DSP_OK;
  HIP_TRY(launch_loop_schedule_prepare(*st, *m, (hipStream_t)hipStream));
  return DSP_OK;
}

// the coupled day-ahead LP of a plant that bids a monotone curve (ABI 19): the blocks as above, and the bounds of the P T ordered-pair
// rows [first_coupling_row, first_coupling_row + P T) of rlo / rhi [B][m_rows], P = S (S - 1) / 2
int dsp_loop_monotone_prepare(const dsp_loop_market_state *st, const dsp_loop_market_model *m, double *rlo, double *rhi, int32_t m_rows,
                              int32_t first_coupling_row, void *hipStream) {
  if (!loop_market_state_ok(st) || !loop_market_model_ok(m) || !rlo || !rhi || st->S < 2 || first_coupling_row < 0) return DSP_ERR_INVALID;
  if ((long long)m->row_stride < (long long)st->S * m->n) return DSP_ERR_INVALID;
  if ((long long)first_coupling_row + (long long)(st->S * (st->S - 1) / 2) * m->T > (long long)m_rows) return DSP_ERR_INVALID;
  if (!loop_market_prepare_ok(st, m) || m->wind_kw_plant || m->c0_base_plant) return DSP_ERR_INVALID;
  if (st->B == 0) return DSP_OK;
  HIP_TRY(launch_loop_monotone_prepare(*st, *m, rlo, rhi, (int)m_rows, (int)first_coupling_row, (hipStream_t)hipStream));
  return DSP_OK;
}

// the coupled real-time LP of a look-ahead hour past midnight (added under ABI 22): the blocks of dsp_loop_schedule_prepare at hour k of
// the day, and - rlo / rhi given - the bounds of the P T ordered-pair rows as dsp_loop_monotone_prepare's, from the real-time prices
int dsp_loop_midnight_prepare(const dsp_loop_market_state *st, const dsp_loop_market_model *m, double *rlo, double *rhi, int32_t m_rows,
                              int32_t first_coupling_row, int32_t k, void *hipStream) {
  if (!loop_market_state_ok(st) || !loop_market_model_ok(m) || k < 0 || k > 23 || 24 - k >= m->T) return DSP_ERR_INVALID;
  if (!st->da_offer || !st->da_prices || !rlo != !rhi) return DSP_ERR_INVALID;
  if ((long long)m->row_stride < (long long)st->S * m->n) return DSP_ERR_INVALID;
  if (rlo && (st->S < 2 || first_coupling_row < 0 ||
              (long long)first_coupling_row + (long long)(st->S * (st->S - 1) / 2) * m->T > (long long)m_rows))
    return DSP_ERR_INVALID;
  if (!loop_market_prepare_ok(st, m) || m->wind_kw_plant || m->c0_base_plant) return DSP_ERR_INVALID;
  if (st->B == 0) return DSP_OK;
  HIP_TRY(launch_loop_midnight_prepare(*st, *m, rlo, rhi, (int)m_rows, (int)first_coupling_row, (int)k, (hipStream_t)hipStream));
  return DSP_OK;
}

int dsp_loop_market_clear(const dsp_loop_market_state *st, const dsp_loop_market_model *m, const dsp_loop_model *tr, int32_t k, int32_t T,
                          double *dispatch, int32_t *curve, int32_t *count, void *hipStream) {
  if (!loop_market_state_ok(st) || !loop_market_model_ok(m) || k < -1 || k > 23 || T < 1 || T > m->T) return DSP_ERR_INVALID;
  if (st->coupled && (long long)m->row_stride < (long long)st->S * m->n) return DSP_ERR_INVALID;      // (ABI 19: the S blocks of a row)
  if (!m->x || !m->status || !dispatch || !curve || !count) return DSP_ERR_INVALID;
  if (k < 0 ? (T > 24 || !st->da_prices || tr) : T > DSP_LOOP_MAX_T) return DSP_ERR_INVALID;
  if (!plant_sizes_ok(m->wind_kw_plant, m->c0_base_plant, m->wind_cols[0])) return DSP_ERR_INVALID;
  if (k < 0 ? !loop_cols_ok(m->pda_cols, T, m->n) : !loop_terms_ok(m->pt_cols, T, m->n)) return DSP_ERR_INVALID;
  if (tr && (!loop_tracker_ok(tr, T, st->state, st->cf_series) || tr->n_state != m->n_state || !tr->wind_kw_plant != !m->wind_kw_plant)) return DSP_ERR_INVALID;
  if (!plant_p_min_ok(st, (hipStream_t)hipStream)) return DSP_ERR_INVALID;
  if (st->B == 0) return DSP_OK;
  HIP_TRY(launch_loop_market_clear(*st, *m, tr, (int)k, (int)T, dispatch, curve, count, (hipStream_t)hipStream));
  return DSP_OK;
}

// parametrized bidding of the descriptor loop (dsp_param.hip): every index and pointer a lane would use is checked here
int dsp_loop_param_step(const dsp_loop_param_state *st, const dsp_loop_model *tr, int32_t phase, int32_t k, void *hipStream) {
  if (!st || !tr || st->B < 1 || st->N < 24 || tr->T < 1 || tr->T > DSP_LOOP_MAX_T) return DSP_ERR_INVALID;
  if (phase < 0 || phase > 2 || (phase == 0 ? k != -1 : (k < 0 || k > 23))) return DSP_ERR_INVALID;
  if (tr->wind_kw_plant || tr->c0_base_plant) return DSP_ERR_INVALID;      // the parametrized bidders take one wind size (wind_mw)
  if (!st->start || !st->hour || !st->da_series || !st->rt_series || !st->da_cf_series || !st->rt_cf_series || !st->bid_price ||
      !st->storage_mw)
    return DSP_ERR_INVALID;
  if (phase == 0) {
    if (!st->da_offer || !st->da_prices || !st->da_curve || !st->da_count) return DSP_ERR_INVALID;
  } else if (phase == 1) {
    if (!st->rt_dispatch || !st->rt_curve || !st->rt_count) return DSP_ERR_INVALID;
    if (!loop_tracker_ok(tr, tr->T, st->state, st->rt_cf_series)) return DSP_ERR_INVALID;
  } else {
    if (!st->h2_kg || !tr->x || tr->n < 1 || !market_col_ok(st->pem_col, tr->n)) return DSP_ERR_INVALID;
  }
  HIP_TRY(launch_loop_param_step(*st, *tr, (int)phase, (hipStream_t)hipStream));
  return DSP_OK;
}

// the projection tracker of the descriptor loop (dsp_project.hip): every index and pointer a lane would use is checked here
int dsp_loop_project(const dsp_loop_project_state *st, const dsp_loop_model *pj, int32_t phase, int32_t j, void *hipStream) {
  if (!st || st->B < 1 || st->N < 1 || st->ruc_hour < 1 || st->ruc_hour > 23 || phase < 0 || phase > 2) return DSP_ERR_INVALID;
  if (j < 0 || j >= (phase == 2 ? 1 : 24 - st->ruc_hour)) return DSP_ERR_INVALID;
  if (phase == 2) {
    if (!st->da_offer || !st->da_prices || !st->pend_offer || !st->pend_prices || st->slots < 0 || st->slots > DSP_MARKET_MAX_S + 1) return DSP_ERR_INVALID;
    if (st->slots > 0 && (!st->da_curve || !st->da_count || !st->pend_curve || !st->pend_count)) return DSP_ERR_INVALID;
    HIP_TRY(launch_loop_project(*st, pj ? *pj : dsp_loop_model{}, 2, 0, (hipStream_t)hipStream));
    return DSP_OK;
  }
  if (!pj || pj->T < 1 || pj->T > DSP_LOOP_MAX_T || pj->n < 1 || pj->m < 1 || pj->n_state < 0 || pj->n_state > 2) return DSP_ERR_INVALID;
  if (!st->start || !st->hour || (pj->n_state > 0 && (!st->state || !st->proj_state))) return DSP_ERR_INVALID;      // (no state: empty traces may be NULL)
  if (!plant_sizes_ok(pj->wind_kw_plant, pj->c0_base_plant, pj->wind_cols[0])) return DSP_ERR_INVALID;
  if (phase == 0) {
    if (!st->da_offer || !loop_tracker_ok(pj, pj->T, st->state, st->cf_series)) return DSP_ERR_INVALID;
  } else {
    if (!pj->x || !pj->status || !pj->c0 || !st->obj || (pj->n_state > 0 && !st->proj_real) || !st->proj_obj) return DSP_ERR_INVALID;
    for (int e = 0; e < pj->n_state; ++e)
      if (!market_col_ok(pj->state_real[e], pj->n) || !(st->state_scale[e] > 0.0)) return DSP_ERR_INVALID;
  }
  HIP_TRY(launch_loop_project(*st, *pj, (int)phase, (int)j, (hipStream_t)hipStream));
  return DSP_OK;
}

}  // extern "C"
