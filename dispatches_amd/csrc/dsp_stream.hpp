// dsp_stream.hpp — data structures of the HBM-resident ("streaming") batched PDLP (dsp_stream.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/dsp_hip.h"
#include "dsp_prepare.hpp"

namespace dsp {

constexpr int kStreamMaxW = 8;         // ELL width cap: longer vectors go to the long list
constexpr int kStreamMaxLong = 4096;   // long vectors per orientation

// one orientation of the scaled matrix: entry-major ELL ([W][nvec]) + CSR segments of the long vectors
struct StreamMatrix {
  int nvec, W, nlong;
  const double *val;          // [W][nvec]
  const int32_t *idx;         // [W][nvec]
  const uint8_t *is_long;     // [nvec]
  const int32_t *long_id;     // [nlong]   vector id
  const int32_t *long_ptr;    // [nlong+1]
  const int32_t *long_idx;
  const double *long_val;
  int nchunk;                 // chunks of <= 2048 entries over all long vectors
  const int32_t *chunk_begin, *chunk_end;   // [nchunk]   entry range of each chunk
  const int32_t *long_chunk_ptr;            // [nlong+1]  chunks of each long vector
};

// Fused iteration (k_fused): ONE launch per plain iteration for BANDED matrices (the multi-period LPs of the reference: period-
// major columns and rows, every non-long vector touches its own and the neighbouring period).  Rows and columns are cut into
// `ntile` contiguous tiles; a tile's workgroup stages y of its rows (+ the halo rows its columns touch) in LDS, computes the
// primal step of its columns (+ the halo columns its rows touch) into LDS, then the dual step and both Halpern averagings of
// what it owns: xbar never travels through HBM, and x, y are read and written once.  Long columns (design variables that
// touch every period) enter through per-tile partial sums of A^T y that every tile leaves behind for the next launch.
constexpr int kFusedMaxLong = 4;       // long columns the fused form carries (design variables)
struct FusedPlan {
  int ntile = 0;                       // 0 = not applicable (not banded enough, long rows, too many long columns)
  int rows_per_tile = 0;
  int ny_max = 0, nxb_max = 0;         // LDS extents per scenario: staged y rows, xbar slots (long columns first)
  int own_max = 0;                     // most rows or columns any tile owns (k_fused_pre: K = ceil(own_max / 256) per thread)
  int halo_max = 0;                    // most halo rows / columns of any tile (k_fused_pre handles halo columns in one pass: <= 256)
  const int32_t *tile = nullptr;       // [ntile][8]  i0, i1 (own rows), j0, j1 (own columns), c_lo, c_hi, r_lo, r_hi
  const int32_t *ridx_enc = nullptr;   // [R.W][m] row ELL column index; long column l encoded as -1 - l
};

struct StreamProblem {
  int n, m;
  StreamMatrix R, C;          // A (rows) and A^T (columns)
  const double *col_scale, *row_scale;
  FusedPlan F;
};

// per-scenario control block (device memory; written by k_init_control / k_control only)
struct StreamCtrl {
  double w, tau, sig, w_lo, w_hi;
  double r0, rprev;
  double qn, cn, c0, pobj;
  double last_rp, last_rd, last_rg;
  int k, it, status, done, mode, nrestart;
  int suspect;                // the objectives are drifting apart (relative gap >= 1/2 after 2048 iterations): certificate sequence wanted
};

#if defined(__HIPCC__)
// ---- control: the restart / termination decision of one scenario from its check sums (slot layout: k_check_rows / k_kkt_cols of dsp_stream.hip;
// shared with the lane-per-scenario form, dsp_stream_lane.hip)
// returns the mode for the apply step (0 = Halpern step, 1 = restart at (x+, y+)); sets c.done / c.status on termination
__device__ inline int control_decide(const double *acc, StreamCtrl &c, const dsp_options &o, double eta, int iters_this_period) {
  c.it += iters_this_period;
  c.k += iters_this_period;
  const double w = c.w, iw = 1.0 / w;
  const double r = fmax(w * acc[0] + iw * acc[1], 0.0);        // squared fixed-point residual in the PDHG metric
  int mode = 0;
  if (!(r == r)) { c.status = DSP_STATUS_NUMERICAL; c.done = 1; }
  else {
    const double po = acc[9] + acc[7], dobj = acc[4] + acc[10];      // acc[7]: quadratic terms of the soft rows (0 for an LP)
    c.pobj = po;
    const double rp = sqrt(acc[2]) / (1.0 + c.qn), rd = sqrt(acc[8]) / (1.0 + c.cn);
    const double gap = fabs(po - dobj);
    const double rg = gap / (1.0 + fabs(po) + fabs(dobj));
    bool fin;                                                    // same tests as the fused kernel (dsp_kernels.hip)
    if (o.eps_obj > 0.0) {
      const double lim = fmax(o.eps_obj * (1.0 + fabs(po + c.c0)), 1e-12 * acc[11]);
      fin = rp <= o.eps_rel && rd <= o.eps_rel && gap + acc[3] + acc[12] <= lim;
    } else {
      fin = rp <= o.eps_rel && rd <= o.eps_rel && rg <= o.eps_rel;
    }
    c.last_rp = rp; c.last_rd = rd; c.last_rg = rg;
    // An LP without a solution: no fixed point, one of the objectives runs away, the relative gap tends to 1.  A feasible year-long
    // LP passes 1/2 within its first 1.3 - 1.5 k iterations (lab, T = 672 / 1344); a scenario still above it after 2048 is SUSPECT:
    // the host runs the certificate sequence (stream_certify, dsp_stream.hip) on the displacement T(z) - z, at most every 16 checks.
    c.suspect = (o.eps_infeasible > 0.0 && rg >= 0.5 && c.it >= 2048) ? 1 : 0;
    if (fin) { c.status = DSP_STATUS_OPTIMAL; c.done = 1; }
    else if (c.it >= o.max_iter) { c.status = DSP_STATUS_ITERATION_LIMIT; c.done = 1; }
    else {
      const double bs2 = o.restart_sufficient * o.restart_sufficient, bn2 = o.restart_necessary * o.restart_necessary;
      const bool first = !(c.r0 < INFINITY);
      const bool decayed = (r <= bs2 * c.r0) || (r <= bn2 * c.r0 && r > c.rprev);
      const bool artificial = (double)c.k >= o.restart_artificial * (double)c.it;
      if (first) c.r0 = r;
      c.rprev = r;
      if (!first && (decayed || artificial)) {
        double wn = w;
        if (acc[6] > 1e-28 && acc[5] > 1e-28) {
          const double e = log(w) + 0.5 * (log(acc[6]) - log(acc[5]));
          const double dl = fmin(fmax(-o.pid_kp * e, -o.max_dlog_weight), o.max_dlog_weight);
          wn = w * exp(dl);
        }
        wn = fmin(fmax(wn, c.w_lo), fmax(c.w_hi, c.w_lo));
        c.w = wn; c.tau = eta / wn; c.sig = eta * wn;
        c.k = 0; c.r0 = INFINITY; c.rprev = INFINITY;
        c.nrestart += 1;
        mode = 1;
      }
    }
  }
  c.mode = mode;
  return mode;
}

#endif

struct StreamWork {
  double *x, *x0, *xp, *xbar, *c, *lb, *ub;     // [B][n]  scaled space
  double *y, *y0, *yp, *rlo, *rhi, *kap;        // [B][m]   (kap: scaled compliance of the soft rows, QP only)
  double *x2, *y2;                              // [B][n] / [B][m] second buffers of the fused iteration (x / y ping-pong)
  double *lpart[2];                             // [B][nlong][ntile] partial sums of A^T y for the long columns (ping-pong)
  StreamCtrl *ctrl;                             // [B]
  double *partial;                              // [B][nblk_tot][16] ordered block partial sums
  double *long_partial;                         // [B][nchunk_max] chunk partials of the long vectors
  int *ndone;                                   // [2]: scenarios finished; flag "some scenario is suspect" (set by the decision kernels)
  double *ray;                                  // [B][m] scratch of the certificate sequence (the cleaned dual displacement)
};

struct StreamArgs {
  StreamProblem P;
  StreamWork W;
  dsp_batch b;
  dsp_options opt;
  double eta;
  int nblk_n;      // blocks over the columns
  int nblk;        // blocks over max(n, m) elements
  int nblk_tot;    // + blocks of the long vectors (partial-sum stride)
  int nchunk_max;  // stride of long_partial
};

// bounds that are ONE template for the whole batch (stride 0: the price-taker families differ in the objective only)
inline bool batch_bounds_shared(const dsp_batch &b) {
  return (!b.var_lb || b.var_lb_stride == 0) && (!b.var_ub || b.var_ub_stride == 0) && (!b.row_lb || b.row_lb_stride == 0) &&
         (!b.row_ub || b.row_ub_stride == 0);
}
// algorithmic HBM bytes per scenario and plain iteration of the one-launch forms (tile, lane): x, x0, c, y, y0 read, x, y written; bounds
// of its own per scenario and the compliance of soft rows on top
inline size_t one_launch_bytes_per_iteration(size_t n, size_t m, bool shared, bool qp) {
  return (size_t)8 * (shared ? 4 * n + 3 * m : 6 * n + 5 * m) + (qp ? 8 * m : 0);
}

// The cadence of the host-enqueued PDHG forms (two-launch, tile, lane): a check every C iterations, a look at the finished counter every
// kPollPeriods check periods and after the last one, the certificate sequence for suspects at most every kCertifyPeriods.
constexpr int kPollPeriods = 4;
constexpr int kCertifyPeriods = 16;
inline int check_period(const dsp_options &o) { return o.check_every > 0 ? o.check_every : 64; }       // 0 = automatic (include/dsp_hip.h)
inline int max_check_periods(const dsp_options &o) { return (o.max_iter + check_period(o) - 1) / check_period(o); }
inline bool poll_due(int periods_done, int max_periods) { return periods_done % kPollPeriods == 0 || periods_done == max_periods; }
// ndone_host: {scenarios finished, some scenario is suspect (relative gap >= 1/2 after 2048 iterations: control_decide)}
inline bool certify_due(const int *ndone_host, int periods_done) { return ndone_host[1] && periods_done % kCertifyPeriods == 0; }

struct LaneState;                      // lane-per-scenario form (dsp_stream_lane.hip); nullptr = not applicable to this matrix
struct IpmState;                       // interior-point form for time-banded LPs (dsp_ipm.hip); nullptr = not applicable

// What a solve reports (dsp_stats): value-initialised by stream_solve before anything else, then filled in by the form that takes the batch
struct StreamReport {
  int form = 0;                     // DSP_STREAM_FORM_*
  int phases = 0;                   // lane form: its phases; interior point: its time partitions (dsp_stats::stream_phases)
  size_t bytes_per_iteration = 0;   // algorithmic HBM bytes per scenario and plain iteration; 0 = the two-launch figure (stream_bytes_per_iteration)
  int newton = 0;                   // interior-point form: Newton iterations
  int ipm_solved = 0;               // ... and the scenarios it solved (the others went on to the PDHG forms)
};

struct StreamSolver {
  StreamProblem P{};
  StreamWork W{};
  int work_B = 0;
  std::vector<void *> allocs, work_allocs;
  int *ndone_host = nullptr;
  LaneState *lane = nullptr;
  IpmState *ipm = nullptr;
  StreamReport report;    // of the last solve
  std::mutex mu;         // one solve at a time per handle: the workspace above is per handle, not per call (stream_solve)
  size_t lds_limit = 160 * 1024 - 2048;   // dynamic LDS available to the block-resident form (static __shared__ on top)
};

hipError_t stream_create(const HostCSR &A_scaled, const HostCSR &AT_scaled, const double *col_scale_dev,
                         const double *row_scale_dev, StreamSolver *S);
void stream_destroy(StreamSolver *S);
hipError_t stream_solve(StreamSolver *S, const dsp_batch &batch, const dsp_options &opt, double eta, hipStream_t st,
                        int *periods_run);
// per scenario and plain iteration of the form the last solve ran: two launches 8 n + 6 m doubles (dsp_stream.hip, file header); the
// one-launch forms say their own figure (one_launch_bytes_per_iteration); every other form and before any solve: the two-launch figure
inline size_t stream_bytes_per_iteration(const StreamSolver *S) {
  return S->report.bytes_per_iteration ? S->report.bytes_per_iteration : (size_t)8 * (8 * (size_t)S->P.n + 6 * (size_t)S->P.m);
}
// a host vector on the device (at least one element is allocated), the allocation entered in `allocs`
template <class T>
hipError_t stream_up(std::vector<void *> &allocs, const std::vector<T> &v, const T **out) {
  void *d = nullptr;
  hipError_t e = hipMalloc(&d, (v.empty() ? 1 : v.size()) * sizeof(T));
  if (e != hipSuccess) return e;
  allocs.push_back(d);
  if (!v.empty() && (e = hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)) != hipSuccess) return e;
  *out = reinterpret_cast<const T *>(d);
  return hipSuccess;
}

// dsp_stream_lane.hip
hipError_t lane_create(const HostCSR &A_scaled, const HostCSR &AT_scaled, StreamSolver *S);
void lane_destroy(StreamSolver *S);
hipError_t lane_run(StreamSolver *S, StreamArgs &a, hipStream_t st, int *periods_run, bool *used, const std::vector<int> *only = nullptr);
// dsp_ipm.hip: scenarios it solves get ctrl.done = 1 / status 0 and their x+ / y+ in the scenario-major workspace; the others are untouched
hipError_t ipm_create(const HostCSR &A_scaled, const HostCSR &AT_scaled, StreamSolver *S);
void ipm_destroy(StreamSolver *S);
hipError_t ipm_run(StreamSolver *S, StreamArgs &a, hipStream_t st, bool *all_solved, int *newton, int *n_solved);
int ipm_partitions(const StreamSolver *S);     // time partitions of its banded solves (1: sequential walks; 0: no interior-point plan)
// certificate sequence on the scenario-major workspace (x, y = the current iterate): dsp_stream.hip
hipError_t stream_certify(StreamSolver *S, StreamArgs &a, hipStream_t st);

// the device's finished counter and suspect flag into S->ndone_host, after everything enqueued on `st`
inline hipError_t stream_poll(StreamSolver *S, const StreamArgs &a, hipStream_t st) {
  const hipError_t e = hipMemcpyAsync(S->ndone_host, a.W.ndone, 2 * sizeof(int), hipMemcpyDeviceToHost, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}
// The interior-point form solved the batch or part of it (a PDHG form took the rest): the solve is reported as DSP_STREAM_FORM_IPM with
// its time partitions as phases; dsp_stats::ipm_solved says how many it solved.
inline void report_interior_point(StreamSolver *S) {
  if (S->report.ipm_solved > 0) { S->report.form = DSP_STREAM_FORM_IPM; S->report.phases = ipm_partitions(S); }
}

}  // namespace dsp
