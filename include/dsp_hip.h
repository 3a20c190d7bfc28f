/* dsp_hip.h — C ABI of the MI355X batched dispatch-LP solver (libdsp_hip.so).
 *
 * Drop-in seam: the reference has no FFI; its solve boundary is the Python call
 *     solver.solve(model, tee=...)                       (UPSTREAM pyomo SolverFactory object)
 * made from Bidder.compute_day_ahead_bids / compute_real_time_bids and Tracker.track_market_dispatch
 * (reference call sites: dispatches/case_studies/renewables_case/run_double_loop_battery.py:123,222-285,
 *  dispatches/case_studies/renewables_case/tests/test_multiperiod_wind_battery_doubleloop.py:47,81,140,160,235,
 *  dispatches/workflow/parametrized_bidder.py:73-119).  Where Pyomo writes an LP/NL file and spawns
 * cbc / ipopt, a binding of this library hands over the flattened standard form
 *
 *     min c.x + c0   s.t.  row_lb <= A x <= row_ub,   var_lb <= x <= var_ub          (one scenario)
 *
 * or, for the convex QPs of BASELINE config 5 (quadratic ramp cost), the same with SOFT rows (dsp_batch::row_compliance):
 *
 *     min c.x + c0 + sum_{i soft} (a_i.x - b_i)^2 / (2 kappa_i)      s.t. the hard rows and the column bounds
 *
 * once (dsp_create: the CSR of A shared by every scenario) and then, per call, B dense per-scenario vectors
 * (dsp_solve).  Plain C, opaque handle, caller-owned buffers, int return codes, stream-ordered.
 * All per-scenario pointers in dsp_batch / dsp_spmv_step are DEVICE pointers (e.g. torch.Tensor.data_ptr());
 * everything in dsp_lp_desc is a HOST pointer that is copied during dsp_create.
 *
 * The rolling double loops on top of it (dsp_wb_rolling_update, dsp_loop_update, dsp_loop_market_*, dsp_loop_param_step) write the LPs
 * of a simulated hour from device-resident series and state.  ABI 17 adds the reference's day-ahead timeline to the descriptor loop:
 * dsp_loop_project runs the coordinator's projection tracker (bid_into_DAM: the rest of today's cleared day-ahead dispatch tracked to
 * midnight, free dispatch rows past it) and makes the bid computed at the RUC hour current at midnight;
 * dsp_loop_market_state::rt_history_lag_days ages the real-time backcast of that bid by the day that is not complete yet.
 * ABI 18 adds the self-scheduling plant: dsp_loop_schedule_prepare writes ONE coupled day-ahead LP per plant (S scenario blocks side by
 * side in a row, tied by static non-anticipativity rows) and dsp_loop_market_clear reads block 0 of such a row
 * (dsp_loop_market_model::row_stride) and prices the schedule at 0 (dsp_loop_market_state::self_schedule, curve_slots).
 * ABI 19 adds the Bidder's monotone bid curves across price scenarios: dsp_loop_monotone_prepare writes ONE coupled day-ahead LP per plant
 * (the same S blocks, and the bounds of the S (S - 1) / 2 * T ordered-pair rows from the order of the day-ahead scenario prices) and
 * dsp_loop_market_clear reads scenario i of plant b from block i of row b (dsp_loop_market_state::coupled, was reserved).
 * ABI 20 adds the per-plant ledger of the implemented hour: dsp_loop_ledger evaluates up to 8 linear forms (total cost, missed delivery,
 * curtailment, hydrogen, ...) on the tracker's solution and adds them to per-plant accumulators, before phase 2 of dsp_loop_update
 * advances the clock; and dsp_loop_market_state::p_min_cents_plant, a per-plant minimum power of the bid curves (appended; NULL = ABI 19).
 * ABI 21 adds the recorder of the descriptor loop: dsp_loop_record copies up to 16 strided segments (states, solutions, curves, ...) of up
 * to 64 chosen plants into the row of the record that the device clock names - one gather launch, so that the record is written by the
 * replayed hipGraphs too.  Nothing else changes.
 * Added under ABI 22, DSP_VERSION unchanged: dsp_loop_health and dsp_loop_health_state, the per-plant solve health of the descriptor loop
 * (rows solved / failed / waived, status mask, iteration sum and maximum, first failing hour - per plant and kind of solve).  A new symbol
 * and a new struct only: no existing struct, entry point or kernel changed, so a caller of ABI 22 that does not know them is unaffected.
 * Added the same way, DSP_VERSION still 22: dsp_loop_profile (every plant's delivered power kept hour by hour) and the representative
 * days over it - dsp_days_assign, dsp_days_update, dsp_days_frequency, dsp_days_work_doubles with dsp_loop_profile_desc / dsp_days_desc.
 */
#ifndef DSP_HIP_H
#define DSP_HIP_H

#ifndef __HIPCC_RTC__   /* hiprtc has no system headers; the kernel sources define the fixed-width types themselves */
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define DSP_VERSION 22

/* return codes (0 = ok, < 0 = API misuse / HIP error; text via dsp_strerror) */
#define DSP_OK                 0
#define DSP_ERR_INVALID       -1   /* bad argument (NULL, negative size, unsorted CSR, ...)            */
#define DSP_ERR_TOO_LARGE     -2   /* LP beyond what the layouts support (see dsp_strerror)            */
#define DSP_ERR_HIP           -3   /* a HIP runtime call failed (dsp_last_hip_error())                */
#define DSP_ERR_NO_DEVICE     -4   /* no gfx950 device visible                                        */
#define DSP_ERR_ALLOC         -5

/* per-scenario termination status written to status[B] */
#define DSP_STATUS_OPTIMAL            0
#define DSP_STATUS_ITERATION_LIMIT    1
#define DSP_STATUS_PRIMAL_INFEASIBLE  2   /* no point satisfies rows and bounds.  Reported (i) for crossed bounds in the input (var_lb > var_ub or
                                             row_lb > row_ub: before any iteration, x / y / obj = NaN), (ii) by the in-wave simplex when its
                                             phase 1 ends at a certified optimum clearly outside the bounds (x / y / obj = NaN), (iii) by the
                                             PDLP kernels - fused and HBM-resident - when the displacement T(z) - z of the iteration is a
                                             FARKAS RAY to dsp_options::eps_infeasible: a row multiplier dy (signs admitted by the finite row
                                             bounds) whose reduced costs -A'dy are absorbed by finite column bounds and whose bound value
                                             dy+.row_lb - dy-.row_ub + rc+.var_lb - rc-.var_ub is positive (x / y hold the last iterate)       */
#define DSP_STATUS_DUAL_INFEASIBLE    3   /* the objective is unbounded below along a recession direction of the feasible set (or the dual is
                                             infeasible): reported by the PDLP kernels when the primal part dx of the displacement, clipped to
                                             the recession cone of the column bounds, has c.dx < 0 and A dx inside the recession cone of the
                                             rows to dsp_options::eps_infeasible (x / y hold the last iterate).  An LP that is infeasible or
                                             unbounded by a margin below that tolerance still ends at ITERATION_LIMIT                          */
#define DSP_STATUS_NUMERICAL          4   /* NaN in the input or NaN / Inf met in the iteration                */

/* per-scenario flag bits written to flags[B] */
#define DSP_FLAG_OBJ_WAIVED   1   /* status OPTIMAL with both feasibility tests at eps_rel, but the objective-error bound
                                     only within 10 eps_obj (or the classic relative gap at eps_rel): bound AND objective stagnated
                                     (dsp_options::polish_patience) or the iteration stalled twice (stall_rescue).  The 1e-6
                                     objective accuracy is NOT certified for this scenario (measured: still within 3e-7);
                                     typically objectives that are the small difference of terms ~1e3-1e6 times larger   */
#define DSP_FLAG_STALL_RESCUE 2   /* the primal weight was reset once by the stall rescue                              */
#define DSP_FLAG_POLISH       4   /* the weight guard was tightened in the polish phase (dsp_options::polish_patience) */
#define DSP_FLAG_SIMPLEX_KKT  8   /* ABI 22: status OPTIMAL from the in-wave simplex, and the stored (x, y) passed the full KKT certificate
                                     against the ORIGINAL LP at dsp_options::simplex_kkt_tol (dsp_options::simplex_certify = 1) */

typedef struct dsp_handle dsp_handle;

/* One scenario's LP template.  Replaces the model Pyomo would write to disk on every solve. */
typedef struct dsp_lp_desc {
  int32_t n;                 /* columns                                  */
  int32_t m;                 /* rows                                     */
  int64_t nnz;               /* nonzeros of A                            */
  const int32_t *A_rowptr;   /* [m+1]  CSR, column indices ascending within a row */
  const int32_t *A_colidx;   /* [nnz]  */
  const double  *A_val;      /* [nnz]  */
  const double  *col_scale;  /* [n] or NULL: variable scaling factors, the typical magnitude of each column (x_j = s_j x~_j with
                                x~ of order one) - what IDAES models carry as `iscale.set_scaling_factor` (there as 1 / s).  Applied
                                before the library's own equilibration; inputs and outputs stay in the caller's units.  The
                                wind + battery and wind + PEM bidding LPs (kW, MW, kWh of throughput: 3-8 decades) need 20-60 %
                                fewer iterations with the ranges their bounds imply (dispatches_amd/lp.py: implied_column_ranges) */
} dsp_lp_desc;

/* Solver options (restarted, reflected Halpern PDHG with ray jumps).  Fill with
 * dsp_default_options() and override fields. */
typedef struct dsp_options {
  double  eps_rel;           /* relative KKT tolerance: primal and dual residual (and, with eps_obj = 0, the relative
                                gap)                                                      default 1e-9   */
  double  eps_obj;           /* objective accuracy: the error bound |gap| + sum|y||row violation| + sum|dual residual||x|
                                of the returned point is <= eps_obj (1 + |c.x + c0|) - half of the 1e-6 parity contract by
                                default; it replaces the relative-gap test (c.x without the model constant is ~500x the
                                objective here, which made that test a 3x tighter duplicate and the one every straggler
                                hung on).  0 = classic PDLP tests (eps_rel on the relative gap)   default 5e-7   */
  int32_t max_iter;          /* iteration limit per scenario                          default 200000 */
  int32_t check_every;       /* restart / ray-jump test period (1 SpMV + 1 reduction); 0 = automatic: 16, or 32 for LPs with
                                more than 8 owned elements per lane in the fused kernel (the rare blocks of their check spill), 64 on the
                                streaming path                                            default 0      */
  double  restart_sufficient;/* beta_1: restart when r <= beta_1 r0                   default 0.2    */
  double  restart_necessary; /* beta_2: ... or r <= beta_2 r0 and r increased         default 0.8    */
  double  restart_artificial;/* beta_3: ... or k >= beta_3 * total iterations.  0 = automatic: 0.2 in the fused float64
                                kernels (0.3 with soft rows), 0.36 on the streaming / block-resident and float32 paths.
                                Shorter epochs cut the mean iteration count of every flowsheet by 10-28 % (0.36 -> 0.2:
                                profiles/r04j..r04m scans); they also update the weight more often, hence the gentler
                                pid_kp that goes with them                                   default 0      */
  double  pid_kp;            /* proportional gain of the primal-weight controller; 0 = automatic: 0.6 in the fused float64
                                kernels, 0.7 elsewhere (max_dlog_weight = 0 switches the controller off)  default 0 */
  double  max_dlog_weight;   /* clamp on |delta log(primal weight)| per restart       default log(30)*/
  double  step_scale;        /* eta = step_scale / ||A_scaled||_2                     default 0.998  */
  double  weight_guard;      /* keeps the primal weight where step x rounding noise stays below eps / guard:
                                w >= guard eta 1.1e-16 |c|max / (eps (1+|q|)) (and the mirror bound); 0 = off  default 4 */
  double  jump_steady;       /* ray jump: attempt when |r - r_prev| <= jump_steady r  default 0.05   */
  double  jump_tol;          /* ... and ||T(T z)-2T z+z|| <= jump_tol ||T(T z)-T z||  default 3e-3   */
  double  jump_min;          /* ... and the ray stays >= jump_min steps in its piece  default 4      */
  int32_t ray_jumps;         /* 0 = off, 1 = ray jumps, 2 = + chaining (a landing point is tested again at its
                                first check; measured worse on full batches)           default 1      */
  int32_t ruiz_iters;        /* Ruiz passes before Pock-Chambolle (create time)       default 10     */
  int32_t waves_per_block;   /* scenarios per workgroup (1 wave each); 0 = auto                      */
  int32_t kkt_every;         /* the KKT / termination test (7 reductions + two SpMVs) runs at least every
                                kkt_every-th check (kkt_gate = 0: exactly every kkt_every-th)   default 32     */
  int32_t no_matreg;         /* 1 = never use the register-resident-matrix kernel (create time)  default 0 */
  int32_t geo_iters;         /* geometric-mean equilibration passes BEFORE Ruiz (create time): balances
                                unit-mix rows such as P_T[MW] = 1e-3 (G + O)[kW]; helps the tracking LPs and the
                                nuclear flowsheet, hurts wind+battery bidding           default 0      */
  double  kkt_gate;          /* > 0: the KKT test is scheduled from the (free) fixed-point residual r of the restart
                                test: a test that fails by the factor rho = worst criterion / its limit arms the next
                                one for r <= r_now min(1, kkt_gate / rho); the first test runs at the 4th check and
                                kkt_every bounds the gap.  Only moves WHEN termination is detected, never the iterates.
                                0 = fixed cadence                                         default 16     */
  int32_t stall_rescue;      /* > 0: a restart forced by the artificial criterion alone after >= stall_rescue
                                iterations without the residual decaying means the iteration sits on its rounding
                                floor.  The first time, if the primal weight is within 30x of its rounding guard
                                (weight_guard), the movement-ratio controller has driven it away (seen: gap stuck
                                at 1e-7 relative, residuals at 1e-12) and the weight is pulled back to the
                                geometric mean of its value and the initial weight.  From the second time on the
                                eps_obj tests are waived and the scenario terminates on the eps_rel tests alone:
                                an objective that is the difference of terms 1e5 times larger (near-zero-price
                                days) cannot be resolved to eps_obj in double precision.  The threshold matters:
                                scenarios that converge with a weight at the guard do so within ~10 k iterations
                                and a rescue after 1000 slowed ~70 of the 4096 48-h scenarios 10-25x; 4000 (first
                                possible trigger at iteration 4000 / restart_artificial = 11-20 k) touches none of them.  0 = off
                                                                                          default 4000   */
  int32_t no_simplex;        /* 1 = never use the in-wave dense simplex (create time).  LPs with n + m <= 128 and m <= 64
                                (the hourly real-time-bid and tracking LPs: 24 of the 25 solves of a simulated day) are
                                solved by a bounded-variable primal simplex on the dense tableau, one LP per wave,
                                ~(n + m) / 2 pivots instead of thousands of first-order iterations, and the vertex is
                                certified against the original rows; whatever it does not certify falls through to the
                                PDLP kernel in the same call                                  default 0      */
  double  jump_rel;          /* ray jump: ... and the ray stays >= jump_rel * (iterations since the anchor was
                                last reset) steps in its piece.  A jump resets the Halpern anchor; when the pieces
                                are short the solver otherwise jumps at every opportunity (one jump per ~40
                                iterations, thousands per scenario) and never gets the averaged iteration going:
                                such scenarios were the 10-60x stragglers of every batch        default 3    */
  int32_t precision;         /* 0 = float64 everywhere (the parity path).  1 = float32 iterates, matrix and SpMVs with
                                float64 reductions / KKT tests (dsp_qp.hip: one scenario per wave, no ray jumps), for the
                                fp64-vs-fp32 tolerance sweep of BASELINE config 5 - it cannot reach the 1e-6 objective
                                contract on these LPs (bench.py --workload qp_sweep)             default 0    */
  int32_t polish_patience;   /* > 0: once both feasibility tests hold and the objective-error bound is within 10x of its limit,
                                no 2x improvement of the bound for this many iterations starts the near-miss logic: a weight
                                that sits at its rounding guard gets the guard tightened 4x on the noisy side (at most 3
                                times); after 4x this many iterations without improvement a scenario whose primal objective
                                has not moved by more than eps_obj / 10 either is accepted and flagged DSP_FLAG_OBJ_WAIVED.  Such scenarios - rounding
                                floors and slow drifts along nearly flat directions, the primal objective long converged -
                                were the slowest of every batch (30-58 k iterations).  0 = off       default 1024 */
  int32_t no_rtc;            /* 1 = never compile at run time (create time).  An LP without an ahead-of-time register-resident
                                specialisation (other horizons, other flowsheets, QP variants) gets its tight instantiation
                                compiled by hiprtc in dsp_create: 2-3 s once, then a disk cache ($DSP_RTC_CACHE or
                                ~/.cache/dsp_hip, keyed by shape and a hash of the kernel sources).  Needs libhiprtc.so and
                                the kernel sources ($DSP_KERNEL_SRC or csrc/ next to the library) at run time; without them
                                the padded / LDS-matrix ahead-of-time kernels are used (dsp_rtc_message says why)  default 0 */
  int32_t no_interior_point; /* 1 = never use the interior-point form of the HBM-resident path.  LPs of that path whose normal matrix is
                                TIME-BANDED (half-bandwidth <= 8 in the given row order once at most 4 wide columns - design variables,
                                periodic conditions - are set aside: the year-long price-taker LPs) are solved by a primal-dual
                                interior-point method with exact banded factorisations, one lane per scenario (csrc/dsp_ipm.hip): ~100
                                Newton iterations instead of ~75 k first-order iterations; the factorisations and solves run
                                TIME-PARALLEL from 512 rows on (up to 64 partitions of the horizon, their separators as a
                                block-tridiagonal system: csrc/dsp_ipm_seq.hpp; dsp_stats::stream_phases = partitions).  Scenarios it does not finish (free columns,
                                numerical breakdown, 250 iterations or dsp_options::max_iter if smaller) run the PDHG forms - those scenarios only,
                                the ones it solved stay solved (dsp_stats::ipm_solved) -, batches with soft rows as before; statuses
                                2 / 3 come from the PDHG forms.  `iters` counts Newton iterations for scenarios it solved; warm starts
                                (x0 / y0) are ignored by this form                                                     default 0 */
  double  eps_infeasible;    /* > 0: infeasibility / unboundedness certificates (DSP_STATUS_PRIMAL_INFEASIBLE / DUAL_INFEASIBLE, ABI 9).  On
                                an LP without a solution the PDHG operator has no fixed point, T(z) - z tends to a ray, one of the
                                objectives runs away and the relative gap |c.x - dual objective| / (1 + |c.x| + |dual objective|) tends
                                to 1.  A KKT test that finds the gap >= 1/2 after the 8th check (HBM-resident path: after 2048
                                iterations) marks the scenario SUSPECT - no feasible scenario of the reference's bidding LPs is there at
                                that stage, so feasible batches pay one comparison per KKT test.  For suspects the two certificates are
                                evaluated on the displacement (dy as a Farkas ray, dx clipped to the recession cone of the bounds as a
                                direction of unbounded descent: two products + one reduction) and the scenario ends when
                                    |dual residual of the ray| (1 + |bounds|) <= eps_infeasible * (bound value of the ray)        or
                                    |recession violation of A dx| (1 + |c|) <= eps_infeasible * (-c.dx)
                                (scaled space; both are proofs up to the tolerance, whatever the iterate).  Where: the generic (LDS-
                                matrix) kernels at their restarts; the register-resident kernels only watch the gap and hand a scenario
                                that stays suspect over three KKT tests to a second launch of the generic kernel, which continues from
                                its iterate (that launch returns at once when there is no suspect); the HBM-resident path in a
                                certificate sequence the host enqueues at most every 16 check periods while suspects exist.  Reference
                                behaviour: the solver's termination condition, on which the callers act (case_studies/renewables_case/
                                solar_battery_hydrogen.py:451-458).  0 = off                                        default 1e-6 */
  int32_t recertify_passes;       /* N = 1 .. 3 (ABI 11, fused path): scenarios the solve accepted WITHOUT a certified objective accuracy
                                (DSP_FLAG_OBJ_WAIVED) are solved again ON THE DEVICE, from a cold start, under up to N other restart /
                                weight-controller settings; a certified optimum replaces the flagged point and clears the flag, anything
                                else leaves both in place.  Each pass is one more launch that returns at once while no scenario of the
                                batch is flagged.  For callers that never read the flags back between solves - the rolling double loop
                                replays its simulated days from hipGraphs; the reference re-solves nothing, its solver either converges
                                or the run stops (idaes Bidder: `assert_optimal_termination`).  0 = off (a synchronous caller re-solves
                                flagged scenarios itself: hip_solver.HipPdlpSolver)                                  default 0    */
  int32_t simplex_warm;      /* in-wave simplex (tiny LPs): 1 = start every scenario from the final basis of ITS previous solve on this handle where
                                one is saved (the hourly LPs of a plant's rolling loop share one matrix and differ in costs, bounds and right-hand
                                sides: 2 - 4 pivots from the previous hour's basis against ~26 from the slack basis) and save the final basis;
                                2 = start from the slack basis, save (the first hour of a day: bounds the drift of a tableau carried over);
                                a warm attempt that does not end in a certified optimum is repeated from the slack basis.  The caller keeps
                                scenario k the same plant from call to call.  0 = off                                     default 0    */
  int32_t warm_patience;     /* > 0 (ABI 12, fused path): a scenario started from dsp_batch::x0 / y0 / primal_weight that has not terminated after
                                this many iterations starts again from the cold point (x = clamp(0), y = 0, automatic primal weight) inside the
                                same launch; its iteration count goes on.  A warm start shortens the mean of a rolling day-ahead solve
                                (3650 -> 2244 iterations) but a few scenarios per thousand do far worse from yesterday's point than from
                                zero - one plant-day in 16 384 ran into the iteration limit; with a patience of ~1.5 x the cold mean their cost
                                is bounded by patience + a cold solve.  0 = off                                           default 0    */
  int32_t simplex_certify;   /* in-wave simplex (ABI 22): 0 = a vertex the pivot loop calls optimal is checked against its bounds and the original
                                rows (the residual taken before the last refinement of the basic values); its reduced costs and duals are the
                                tableau's.  1 = before status 0 is stored, the stored pair (x after refinement, y) passes a full KKT
                                certificate computed from the ORIGINAL data only - the scaled matrix, the handle's scalings, the caller's c,
                                bounds and row sides; the tableau is used to read y off its slack columns and for nothing else.  Four
                                numbers in the caller's units, each relative to 1 + the largest magnitude it compares (dsp_batch::kkt):
                                  primal    bounds and row_lb <= A x <= row_ub at the stored x (A x recomputed, the slack value is not read)
                                  dual_col  sign conditions of r = c - A'y against the finite sides of var_lb / var_ub
                                  dual_row  sign conditions of y against the finite sides of row_lb / row_ub
                                  gap       |c.x - (y+.row_lb - y-.row_ub + r+.var_lb - r-.var_ub)| over the finite sides
                                all four <= simplex_kkt_tol: status 0 and DSP_FLAG_SIMPLEX_KKT.  Otherwise the paths of a failed row
                                certificate: after a warm start once more from the slack basis; from the slack basis no basis is kept and
                                the PDLP pass takes the scenario and reports its own status and flags.  The row check then uses the
                                residual of the final vertex too.  It proves that (x, y) is optimal to the tolerance; it does NOT prove
                                that x is a vertex (basic) solution                                                       default 0    */
  double  simplex_kkt_tol;   /* tolerance of the four numbers above; 0 = 1e-9, the level of the row certificate        default 0    */
} dsp_options;

/* The per-call data of B scenarios.  c is required; every other input may be NULL (= no bound: -inf / +inf,
 * offset 0) and each has its own scenario stride in ELEMENTS: stride 0 broadcasts one template vector to all
 * scenarios, stride n (or m, or 1 for obj_offset) is a dense array.  x0 / y0 (optional warm start) and x / y use
 * dense strides n / m. */
typedef struct dsp_batch {
  int32_t B;
  int32_t reserved;
  const double *c;          int64_t c_stride;
  const double *var_lb;     int64_t var_lb_stride;
  const double *var_ub;     int64_t var_ub_stride;
  const double *row_lb;     int64_t row_lb_stride;
  const double *row_ub;     int64_t row_ub_stride;
  const double *obj_offset; int64_t obj_offset_stride;  /* c0: only used to scale the eps_obj tests */
  /* NULL = LP.  Otherwise [m] (stride 0) or [B][m] (stride m) compliances kappa_i >= 0.  A row with kappa_i > 0 is SOFT:
     it needs row_lb = row_ub = b_i (finite) and is not a constraint but the objective term (a_i.x - b_i)^2 / (2 kappa_i)
     - a convex quadratic objective x'Qx / 2 in FACTORED form, Q = sum_i a_i a_i' / kappa_i (the ramp cost
     (rho / 2) sum_t (P_T[t] - P_T[t-1])^2 is T - 1 such rows with kappa = 1 / rho).  By convex duality the term is an equality row
     whose multiplier pays kappa_i y_i^2 / 2, so the solver's dual step of that row becomes the proximal step
     y+ = (y - sigma (a_i.xbar - b_i)) / (1 + sigma kappa_i) and nothing else changes; y_i = -(a_i.x - b_i) / kappa_i at the
     optimum, obj[] includes the quadratic term.  (SURVEY.md 8(b) proposed Q in CSR; a general Q would need a proximal
     step with Q in the PRIMAL, which was measured 10-20x slower on these problems: tools/pdqp_proto.py.)
     Fused kernels (no vectors longer than the ELL width; the in-wave simplex is skipped) and the HBM-resident streaming path. */
  const double *row_compliance; int64_t row_compliance_stride;
  const double *x0;         /* [B][n] or NULL */
  const double *y0;         /* [B][m] or NULL */
  double  *primal_weight;   /* [B] in/out or NULL: > 0 on entry = initial primal weight of the scenario (rolling-
                               horizon carry-over), anything else = automatic; holds the final weight on exit */
  double  *x;               /* [B][n]  primal solution                                              */
  double  *y;               /* [B][m]  row duals (sign: y >= 0 active lower side, y <= 0 upper)     */
  double  *obj;             /* [B]     c.x at the returned x (the caller adds its own c0)           */
  int32_t *status;          /* [B]     DSP_STATUS_*                                                 */
  int32_t *iters;           /* [B] or NULL   iterations used                                        */
  int32_t *jumps;           /* [B] or NULL   ray jumps taken                                        */
  int32_t *flags;           /* [B] or NULL   DSP_FLAG_* bits of the scenario's solve                */
  double  *kkt;             /* [B][4] or NULL (ABI 22, needs dsp_options::simplex_certify = 1): primal, dual_col, dual_row, gap of
                               the in-wave simplex' certificate for every scenario it gave a verdict on - those it rejected and
                               left to the PDLP pass included, which does not touch them -, four NaNs where it ended without a
                               vertex (NaN input, crossed bounds, pivot limit, phase-1 stops, empty ratio tests) or did not run */
} dsp_batch;

/* Aggregate statistics of one dsp_solve call (filled after the call's stream work completes when
 * `sync_stats` is non-zero; otherwise only the launch geometry is filled). */
typedef struct dsp_stats {
  int64_t total_iterations;  /* sum over scenarios                                  */
  int32_t max_iterations;    /* slowest scenario                                    */
  int32_t n_optimal;         /* scenarios with status 0                             */
  int32_t grid_blocks;       /* launch geometry                                     */
  int32_t block_threads;
  int32_t lds_bytes;         /* dynamic LDS per block                               */
  int32_t cols_per_lane;     /* CPL template parameter chosen                       */
  int32_t rows_per_lane;     /* RPL template parameter chosen                       */
  float   kernel_ms;         /* hipEvent time of the solve kernel on `stream` (sync_stats only) */
  int32_t matreg;            /* 1 = the register-resident-matrix specialisation ran          */
  int32_t lds_conflicts_identity; /* simulated extra LDS cycles per iteration of the gathers, identity layout */
  int32_t lds_conflicts_chosen;   /* ... with the slot permutation chosen at create time          */
  int32_t simplex;                /* 1 = the in-wave simplex pass ran first (iters[] then counts pivots for the
                                     scenarios it solved)                                           */
  int32_t streaming;              /* 1 = LP beyond the register/LDS-resident kernels (n > 640 or m > 384): the HBM-resident
                                     PDLP ran (state streamed from HBM every iteration: dsp_stream.hip)    */
  int64_t stream_bytes_per_iteration;  /* streaming path: algorithmic HBM bytes per scenario and plain iteration OF THE FORM THAT RAN
                                          (stream_form): 8 (4 n + 3 m) one-launch forms with shared bounds, 8 (6 n + 5 m) with
                                          per-scenario bounds, 8 (8 n + 6 m) two-launch form (+ 8 m with soft rows)             */
  int32_t quadratic;              /* 1 = soft rows present (QP variant of the kernel ran)                */
  int32_t precision;              /* precision the iterates were held in (dsp_options::precision)        */
  int32_t rtc;                    /* 1 = the kernel that ran was compiled at run time for this LP's shape (dsp_options::no_rtc) */
  int32_t stream_form;            /* streaming path, which form of the iteration ran (ABI 7; was reserved): DSP_STREAM_FORM_* */
  int32_t stream_phases;          /* streaming path, lane form (ABI 8): phases the solve ran in = 1 + the number of times the scenarios
                                     still iterating were packed into fewer groups of 64 lanes after others had finished; interior-point form
                                     (round 5): the time partitions its banded factorisations and solves ran in (1 = sequential walks);
                                     0 otherwise */
  int32_t ipm_solved;             /* streaming path (ABI 11): scenarios the interior-point form solved.  stream_form = DSP_STREAM_FORM_IPM with
                                     ipm_solved < B: the others (given up on: an LP without a solution, a breakdown) were handed - they
                                     alone, packed into as few lane groups as they need - to the PDHG forms, whose statuses and
                                     certificates they carry; iters[] counts Newton iterations for the former, PDHG iterations for the latter */
  int32_t simplex_unsolved;       /* ABI 22 (was reserved): scenarios the in-wave simplex pass left to the PDLP pass (sync_stats only) */
} dsp_stats;

/* dsp_stats::stream_form */
#define DSP_STREAM_FORM_NONE       0   /* not the streaming path */
#define DSP_STREAM_FORM_TWO_LAUNCH 1   /* k_primal + k_dual_halpern per iteration: 8 n + 6 m doubles per scenario-iteration */
#define DSP_STREAM_FORM_TILE       2   /* round 3: one launch per iteration, a workgroup per tile of rows x 2 scenarios (k_fused_pre / k_fused) */
#define DSP_STREAM_FORM_LANE       3   /* round 4: scenario-minor storage, a lane per scenario walks a tile (k_lane; batches of 32 scenarios and more) */
#define DSP_STREAM_FORM_BLOCK      4   /* mid-size LPs: the whole solve in one launch, one workgroup per scenario, state in LDS (k_block_solve) */
#define DSP_STREAM_FORM_IPM        5   /* round 5: interior point with banded LDL' factorisations, one lane per scenario (csrc/dsp_ipm.hip) */

void dsp_default_options(dsp_options *opt);

/* Build the shared, device-resident problem data for one (flowsheet, horizon): diagonal preconditioner
 * (Ruiz + Pock-Chambolle), scaled A in lane-major ELL + long-vector form for A and A^T, step size.
 * `opt` may be NULL. */
int dsp_create(const dsp_lp_desc *desc, int device, const dsp_options *opt, dsp_handle **out);

/* Solve the B scenarios of `batch`.  hipStream: a hipStream_t (NULL = default stream).  The call enqueues
 * work and returns; if `stats` is non-NULL and sync_stats != 0 it synchronises the stream and fills the
 * statistics.  `opt` may be NULL (= the options given to dsp_create).
 * Fused kernels and in-wave simplex (n <= 640, m <= 384): stream-ordered, capturable into a hipGraph, several calls of one
 * handle may be in flight on different streams.  HBM-resident streaming path (larger LPs, dsp_stats::streaming): BLOCKING and
 * one call at a time per handle - the per-scenario state (13 vectors of n / m doubles per scenario) is a per-handle
 * workspace and the host polls a finished-counter while it enqueues the iteration launches; concurrent callers are
 * serialised by a mutex inside the handle, the call returns after its stream work has completed, and it cannot be captured
 * into a hipGraph. */
int dsp_solve(dsp_handle *h, const dsp_batch *batch, const dsp_options *opt, dsp_stats *stats, int sync_stats,
              void *hipStream);

/* The PDLP SpMV step in streaming form (vectors in HBM): AX[B][m] = A X[b],  ATY[B][n] = A^T Y[b] with the
 * UNSCALED A.  This is the kernel the HBM roofline of SURVEY.md 8(d) is quoted on
 * (bytes = B*2*8*(n+m) + shared CSR).  A MEASUREMENT entry point - no solve calls it - compiled for the LP shapes of the benchmark
 * workloads (wind + battery 24 / 48 h, nuclear 24 / 48 h, wind + PEM 48 h); DSP_ERR_INVALID for any other LP, DSP_ERR_TOO_LARGE for
 * an LP of the streaming path (whose iteration kernels are its own: csrc/dsp_stream*.hip). */
int dsp_spmv_step(dsp_handle *h, int32_t B, const double *X, const double *Y, double *AX, double *ATY,
                  void *hipStream);

/* Rolling-horizon hand-off of the wind + battery double loop ON THE DEVICE (reference: MultiPeriodWindBattery.update_model,
 * wind_battery_double_loop.py:181-274, and Bidder._pass_price_forecasts, done per plant and hour by Python there): one launch
 * rewrites the per-plant objective entries, the mutable bounds and the realised state of B plants between two solves.
 * All pointers are DEVICE pointers; `model` describes one of the hourly LPs (real-time bidding / tracking model). */
typedef struct dsp_wb_model {
  double *c, *lb, *ub, *rlo, *rhi;     /* [B][n] / [B][m] per-plant vectors of the LP (the dsp_batch inputs of its solves)     */
  const double *base_c;                /* [n]  cost vector without prices                                                      */
  const double *x;                     /* [B][n] solution of its last solve                                                    */
  int32_t n, m, T;                     /* columns, rows, horizon (T <= 8)                                                      */
  int32_t soc_init, thr_init;          /* columns fixed to the realised state of charge / energy throughput                   */
  int32_t soc0, thr0;                  /* columns holding the state after the first period                                    */
  int32_t wind_cols[8];                /* wind production column of every period (upper bound = availability)                 */
  int32_t pt_cols[8][2];               /* P_T[t] = 1e-3 (x[a] + x[b])                                                          */
  int32_t pda_cols[8];                 /* day-ahead power column of every period (bidding models), -1 otherwise               */
  int32_t track_rows[8];               /* dispatch rows (tracking model), -1 otherwise                                        */
  double wind_kw;
  double *c0;                          /* [B] objective constant of every plant (dsp_batch::obj_offset of its solves) or NULL    */
  double c0_base, waste_per_kw;        /* c0 = c0_base + waste_per_kw * sum_t (wind availability of period t)   (ABI 11)         */
  const int32_t *status, *flags;       /* [B] outputs of its last solve or NULL: the phase after the solve folds them into
                                          dsp_wb_state::bad / uncertified (ABI 11; six tensor launches per solve otherwise)       */
} dsp_wb_model;

typedef struct dsp_wb_state {
  int32_t B, N;                        /* plants; length of the price / capacity-factor series                                */
  const int64_t *start;                /* [B] first hour of every plant's year in the series                                  */
  int64_t *hour;                       /* [1] the clock (hours since the start): advanced by phase 2                         */
  const double *da_series, *rt_series, *cf_series;   /* [N]                                                                   */
  double *soc, *thr;                   /* [B] realised state                                                                  */
  const double *da_offer, *da_prices;  /* [B][24] cleared day-ahead dispatch and prices of the current day                    */
  double *delivered, *revenue, *energy_mwh;          /* [B]                                                                   */
  uint8_t *bad;                        /* [1] or NULL: set to 1 when a solve left a status other than optimal                     */
  int64_t *uncertified;                /* [1] or NULL: + the scenarios a solve left flagged DSP_FLAG_OBJ_WAIVED                   */
} dsp_wb_state;

/* phase 0: before the real-time bidding solve of hour-of-day k  (prices, state, wind availability, day-ahead power fixed to the
 *          cleared dispatch for the hours of the horizon inside the cleared day) on `rt`;
 * phase 1: between the solves: real-time offer = SCED dispatch (stub market) -> dispatch rows, state and wind of `tr`;
 * phase 2: after the tracking solve: delivered power, realised state rounded to 2 dp, revenue, energy, clock + 1. */
int dsp_wb_rolling_update(const dsp_wb_state *st, const dsp_wb_model *rt, const dsp_wb_model *tr, int32_t phase, int32_t k,
                          void *hipStream);

/* The same hour-by-hour hand-off for ANY flowsheet of the reference, described instead of hard-coded (round 6; dispatches_amd/rolling_flowsheets.py):
 * power output P_T[t] = sum_e pt_coef[t][e] x[pt_cols[t][e]] + pt_const[t] (<= 2 terms per period: every P_T of the reference is one or two
 * columns - wind_battery_double_loop.py:175, wind_PEM_double_loop.py:172, nuclear_flowsheet_multiperiod_class.py:211), up to two state
 * columns re-fixed to the tracker's realised values rounded to `state_scale` (100: 2 dp, wind + battery :194-200; 1: an integer, the nuclear
 * tank holdup :232; none: wind + PEM), optional wind availability columns with their curtailment constant, horizons up to 16 periods. */
#define DSP_LOOP_MAX_T 16
typedef struct dsp_loop_model {
  double *c, *lb, *ub, *rlo, *rhi;     /* [B][n] / [B][m] per-plant vectors of the LP                                             */
  const double *base_c;                /* [n] cost vector without prices                                                          */
  const double *x;                     /* [B][n] solution of its last solve                                                       */
  double *c0;                          /* [B] objective constant of every plant (dsp_batch::obj_offset)                           */
  int32_t n, m, T, n_state;
  int32_t pt_cols[16][2];  /* -1 = no such term                                                                       */
  double  pt_coef[16][2];
  double  pt_const[16];
  int32_t pda_cols[16];    /* day-ahead power column of every period (bidding models), -1 otherwise                   */
  int32_t track_rows[16];  /* dispatch rows (tracking model), -1 otherwise                                            */
  int32_t wind_cols[16];   /* wind production column of every period, -1 = the flowsheet has no wind                  */
  int32_t state_init[2], state_real[2];/* columns fixed to the realised state / holding it after the first period                */
  double  wind_kw, c0_base, waste_per_kw;
  const int32_t *status, *flags;       /* [B] outputs of its last solve or NULL (as dsp_wb_model)                                 */
  const double *wind_kw_plant, *c0_base_plant;       /* [B] per PLANT, both or neither (ABI 16): plant b's wind capacity and its
                                          objective constant instead of the scalars wind_kw / c0_base; NULL = the scalars.  Only
                                          with wind columns; `rt` and `tr` of one call carry them together                        */
} dsp_loop_model;

typedef struct dsp_loop_state {
  int32_t B, N;
  const int64_t *start;                /* [B]                                                                                    */
  int64_t *hour;                       /* [1] the clock: advanced by phase 2                                                      */
  const double *da_series, *rt_series, *cf_series;   /* [N] (cf_series NULL without wind)                                         */
  double *state;                       /* [B][n_state] realised state                                                             */
  double state_scale[2];
  const double *da_offer, *da_prices;  /* [B][24]                                                                                */
  double *delivered, *revenue, *energy_mwh;          /* [B]                                                                       */
  uint8_t *bad;                        /* as dsp_wb_state                                                                         */
  int64_t *uncertified;
} dsp_loop_state;

/* phases as dsp_wb_rolling_update: 0 before the real-time bidding solve of hour-of-day k, 1 between the solves, 2 after the tracking solve.
 * Per-plant pointers (ABI 16): refusals as stated at dsp_loop_market_clear. */
int dsp_loop_update(const dsp_loop_state *st, const dsp_loop_model *rt, const dsp_loop_model *tr, int32_t phase, int32_t k, void *hipStream);

/* The ledger of the implemented hour (ABI 20; rolling_flowsheets.py::BatchedDoubleLoop(ledger=True)): n_forms linear forms over the
 * tracker's solution x of plant b, each added to an accumulator of its own.  Called AFTER the tracking solve and BEFORE phase 2 of
 * dsp_loop_update (which advances *st->hour and overwrites the state).  Form f of plant b, with E = n_terms[f] and
 * coef_f = coef + b * coef_stride + f * DSP_LEDGER_MAX_TERMS, in this fixed order (every step rounded once):
 *     v = constant[b * const_stride + f]
 *     v = fma(coef_f[e], x[b][cols[f][e]], v)            for e = 0 .. E - 1
 *     v = fma(per_avail[f], avail0, v)                   only if per_avail[f] != 0
 *     hour_value[f * B + b] = v ;  acc[f * B + b] = acc[f * B + b] + v
 * avail0 = kw * cf_series[(start[b] + *hour) % N] (the product rounded on its own) is the wind available to plant b in the implemented
 * hour, kw = tr->wind_kw_plant[b] where that pointer is set, tr->wind_kw otherwise.  coef_stride / const_stride = 0: one set of
 * coefficients / constants for all plants; otherwise the distance in doubles between two plants' sets (sized wind batches carry
 * per-plant constants, a batch of different hydrogen prices per-plant coefficients).  One lane per (form, plant), plant fastest. */
#define DSP_LEDGER_MAX_FORMS 8
#define DSP_LEDGER_MAX_TERMS 8
typedef struct dsp_loop_ledger_desc {
  int32_t n_forms, reserved;           /* 1 .. DSP_LEDGER_MAX_FORMS; reserved = 0                                                  */
  int32_t n_terms[8];                  /* 0 .. DSP_LEDGER_MAX_TERMS terms of form f                                                */
  int32_t cols[8][8];                  /* column of term e of form f in [0, tr->n); entries past n_terms[f] are not read           */
  double  per_avail[8];                /* factor of avail0 in form f (0: none; needs wind columns in `tr` and st->cf_series)       */
  const double *coef;                  /* [n_forms][8] (coef_stride = 0) or plant b's set at coef + b * coef_stride                */
  const double *constant;              /* [n_forms] (const_stride = 0) or plant b's at constant + b * const_stride                 */
  int64_t coef_stride, const_stride;   /* 0, or >= n_forms * 8 / >= n_forms                                                        */
  double *acc;                         /* [n_forms][B] running sums                                                                */
  double *hour_value;                  /* [n_forms][B] the values of the last booked hour                                          */
} dsp_loop_ledger_desc;

/* DSP_ERR_INVALID, nothing launched and nothing written, for: a NULL st / tr / ledger; B < 0; tr->n < 1 or a NULL tr->x; n_forms outside
 * 1 .. DSP_LEDGER_MAX_FORMS or n_terms[f] outside 0 .. DSP_LEDGER_MAX_TERMS; reserved != 0; a column outside [0, tr->n); a NULL acc,
 * hour_value, coef or constant; a stride that is negative or shorter than one plant's set; per_avail[f] != 0 (or not finite) without wind
 * columns in `tr` (tr->wind_cols[0] < 0), without st->cf_series / st->start / st->hour, or with N < 1.  B = 0 is DSP_OK and no launch.
 * Capturable: one kernel launch on hipStream, no allocation, no synchronisation. */
int dsp_loop_ledger(const dsp_loop_state *st, const dsp_loop_model *tr, const dsp_loop_ledger_desc *ledger, void *hipStream);

/* The recorder of the descriptor loop (ABI 21; rolling_flowsheets.py::BatchedDoubleLoop(record=(plants, days))): a pure gather - no
 * arithmetic, no atomics, no LDS - of n_segments strided buffers of n_plants chosen plants into ONE row of the record.  With
 *     t = *clock + offset ;   r = t / divisor  if  t >= 0 and t / divisor < rows,   r = rows  otherwise (the SPARE row)
 * element j of recorded plant q of segment g is read at  src + plants[q] * plant_stride + j * elem_stride  and written at
 * dst + (r * n_plants + q) * width + j  (all in elements of elem_bytes bytes).  So every dst holds rows + 1 rows of n_plants * width
 * elements, and whatever falls outside the recorded span - the hours after it, the hour "-1" of offset -1 at clock 0 - lands in the spare
 * last row, never out of bounds (the rule of rolling.py::_record).  The two strides let a source be plant-major ([B][width]: plant_stride
 * = its row length, elem_stride = 1) or plant-minor (the ledger's [F][B]: plant_stride = 1, elem_stride = B).  One lane per element,
 * the segment is blockIdx.y (descriptor reads are wave-uniform), consecutive lanes take consecutive j of one plant. */
#define DSP_RECORD_MAX_PLANTS 64
#define DSP_RECORD_MAX_SEGMENTS 16
#define DSP_RECORD_MAX_WIDTH 1048576
typedef struct dsp_loop_record_segment {
  const void *src;                     /* the live buffer                                                                         */
  void *dst;                           /* [rows + 1][n_plants][width] of the record                                               */
  int64_t plant_stride, elem_stride;   /* in elements, each 1 .. 2^40                                                             */
  int32_t width, elem_bytes;           /* 1 .. DSP_RECORD_MAX_WIDTH elements per plant; 4 or 8 bytes each                         */
} dsp_loop_record_segment;
typedef struct dsp_loop_record_desc {
  int32_t n_plants, n_segments;        /* 1 .. DSP_RECORD_MAX_PLANTS; 1 .. DSP_RECORD_MAX_SEGMENTS                                */
  int32_t plants[64];                  /* strictly increasing, in [0, B): held by value so that the entry point checks every one  */
  const int64_t *clock;                /* [1] device: the loop's clock (dsp_loop_state::hour) or the clock of a bid               */
  int32_t divisor, offset;             /* 1 = an hourly record, 24 = a daily one (1 .. 8784); 0, or -1 = the hour just ended      */
  int32_t rows, reserved;              /* the span, 1 .. 2^24 (dst has one more); reserved = 0                                    */
  dsp_loop_record_segment segments[16];
} dsp_loop_record_desc;

/* B is the number of plants of the batch the sources belong to.  DSP_ERR_INVALID, nothing launched and nothing written, for: a NULL rec or
 * rec->clock; B < 1; n_plants outside 1 .. DSP_RECORD_MAX_PLANTS; n_segments outside 1 .. DSP_RECORD_MAX_SEGMENTS; rows outside 1 .. 2^24;
 * divisor outside 1 .. 8784; an offset other than 0 or -1; reserved != 0; plants that are not strictly increasing, or one outside [0, B);
 * in a used segment a NULL src or dst, a width outside 1 .. DSP_RECORD_MAX_WIDTH, an elem_bytes other than 4 or 8, a plant_stride or
 * elem_stride outside 1 .. 2^40.  (That the sources hold B plants at these strides is the caller's statement, as for every buffer of this
 * interface.)  Capturable: one kernel launch on hipStream, no allocation, no synchronisation, no memset. */
int dsp_loop_record(const dsp_loop_record_desc *rec, int32_t B, void *hipStream);

/* The solve health of the descriptor loop (added under ABI 22; rolling_flowsheets.py::BatchedDoubleLoop(health=True)): after every solve of
 * the loop, what its rows' status / flags / iters say is booked to the PLANT the rows belong to, under the KIND of the solve.  A solve with
 * R = rows_per_plant rows per plant books rows b * R .. b * R + R - 1 to plant b (R = S for the independent bidding batches, 1 for a coupled
 * day-ahead row, a self-schedule's hourly LP and the trackers): the rows whose status and flags feed dsp_loop_state::bad / uncertified.
 * With at = kind * B + b, over the rows i of plant b in the order of i:
 *     solves[at] += R ;   fail[at] += #(status != 0) ;   status_mask[at] |= 1 << status   (status 1 .. 29; another non-zero value: bit 30)
 *     waived[at] += #(status == 0 and flags & DSP_FLAG_OBJ_WAIVED)                          (flags  NULL: untouched)
 *     iters[at]  += sum of iters ;   iters_max[at] = max(iters_max[at], max of iters)      (iters  NULL: untouched)
 *     first[b]    = *clock + 1   if first[b] == 0 and a row of b failed                     (0 = none yet: zeroing is the reset)
 * One lane per plant, 256 lanes per block; a lane reads the clock once and updates its own seven entries with plain vector stores: no
 * atomics, no LDS, no cross-lane traffic, integer arithmetic only.  The rows of the other kinds are not touched. */
#define DSP_HEALTH_KINDS 4             /* 0 day_ahead, 1 real_time, 2 tracking, 3 projection                                        */
#define DSP_HEALTH_MAX_ROWS 16         /* rows per plant of one solve (DSP_MARKET_MAX_S)                                            */
typedef struct dsp_loop_health_state {
  int32_t B, reserved;                 /* plants, >= 1; reserved = 0                                                                */
  const int64_t *clock;                /* [1] device: the loop's clock (dsp_loop_state::hour)                                       */
  int32_t *solves, *fail, *status_mask, *waived;     /* [DSP_HEALTH_KINDS][B]                                                       */
  int64_t *iters;                      /* [DSP_HEALTH_KINDS][B] sum of dsp_batch::iters (PDHG iterations or simplex pivots)         */
  int32_t *iters_max;                  /* [DSP_HEALTH_KINDS][B] their maximum                                                       */
  int64_t *first;                      /* [B] clock + 1 at the plant's first non-optimal row of any kind; 0 = none                  */
  int64_t reserved2[4];                /* 0                                                                                         */
} dsp_loop_health_state;

/* status / flags / iters: DEVICE arrays [B * rows_per_plant] of the solve that has just finished (dsp_batch::status / flags / iters).
 * DSP_ERR_INVALID, nothing launched and nothing written, for: a NULL h or status; B < 1; rows_per_plant outside 1 .. DSP_HEALTH_MAX_ROWS;
 * kind outside 0 .. DSP_HEALTH_KINDS - 1; a NULL clock or counter; reserved != 0.  The descriptor travels by value (<= 4 KB).
 * Capturable: one kernel launch on hipStream, no allocation, no synchronisation, no memset. */
int dsp_loop_health(const dsp_loop_health_state *h, const int32_t *status, const int32_t *flags, const int32_t *iters,
                    int32_t rows_per_plant, int32_t kind, void *hipStream);

/* The day profiles of the descriptor loop (added under ABI 22; rolling_flowsheets.py::BatchedDoubleLoop(profiles=days)): the delivered
 * power of EVERY plant, hour by hour, plant-minor - what the reference's market-surrogate workflow cuts into days and clusters
 * (dispatches/workflow/train_market_surrogates/dynamic/).  Launched once after the hand-off of every hour step:
 *     h = *clock - 1 ;  day = min(h / 24, days) ;  profile[(day * 24 + h % 24) * B + b] = delivered[b]
 * Row `days` is the spare row for hours past the span (and for a clock < 1: hour 0 of the spare row) - the recorder's rule.  One lane per
 * plant, 256 lanes per block, one load and one store per lane: no arithmetic, no atomics, no LDS. */
typedef struct dsp_loop_profile_desc {
  int32_t B, days;                     /* plants, >= 0; days of the span, >= 1                                                      */
  const int64_t *clock;                /* [1] device: the loop's clock (dsp_loop_state::hour), already advanced by the hand-off     */
  const double *delivered;             /* [B] device: dsp_loop_state::delivered                                                     */
  double *profile;                     /* [days + 1][24][B] device, MW                                                              */
  int64_t reserved[4];                 /* 0                                                                                         */
} dsp_loop_profile_desc;

/* DSP_ERR_INVALID, nothing launched and nothing written, for: a NULL descriptor, clock, delivered or profile; B < 0; days < 1 or
 * days > DSP_DAYS_MAX_DAYS; B above DSP_DAYS_MAX_PLANTS; reserved != 0.  B == 0: DSP_OK, nothing launched.
 * Capturable: one kernel launch on hipStream, no allocation, no synchronisation, no memset. */
int dsp_loop_profile(const dsp_loop_profile_desc *p, void *hipStream);

/* Representative days (added under ABI 22; dispatches_amd/representative_days.py): the profile cut into day POINTS, one per (day, plant),
 * point p = day * B + b, with F = 24 * channels features.  Every operation is rounded on its own, nothing is contracted into an fma:
 *     channel 1   cf[h] = (profile[day][h][b] - p_min[b]) / (p_max[b] - p_min[b])                          h = 0 .. 23
 *     channel 2   w[h]  = cf_series[(start[b] + 24 * day + h) mod N]   (the realised window; computed on the fly)
 *     class       only with filter: s = ((cf[0] + cf[1]) + ...) + cf[23];  s == 0.0: a zero day, label -1;  s == 24.0: a full day, label -2
 *     distance    for k = 0 .. K - 1: acc = 0; for j = 0 .. F - 1: d = x[j] - c[k][j]; acc = acc + d * d.   label = the first k with the
 *                 smallest acc (strict <); dist2 = that acc.  A zero or full day gets dist2 = 0.
 * p_max[b] > p_min[b] is the caller's contract (a device array cannot be checked on the host). */
#define DSP_DAYS_MAX_K 64              /* centres: K * F doubles are staged in LDS, at most 24 KiB                                   */
#define DSP_DAYS_MAX_DAYS 65536
#define DSP_DAYS_MAX_PLANTS (1 << 24)
#define DSP_DAYS_MAX_POINTS 2147483647 /* B * days                                                                                  */
#define DSP_DAYS_CHUNK 1024            /* points per partial sum of dsp_days_update                                                 */
typedef struct dsp_days_desc {
  int32_t B, days;                     /* plants, >= 0; days, >= 1: the first `days` rows of the profile                            */
  int32_t channels, filter;            /* 1 or 2; 0 or 1                                                                            */
  const double *profile;               /* [>= days][24][B] device, MW                                                               */
  const double *p_min, *p_max;         /* [B] device, MW                                                                            */
  const double *cf_series;             /* [N] device (channels == 2; else ignored)                                                  */
  const int64_t *start;                /* [B] device (channels == 2; else ignored)                                                  */
  int64_t N;                           /* >= 1 (channels == 2; else ignored)                                                        */
  int64_t reserved[4];                 /* 0                                                                                         */
} dsp_days_desc;

/* Every entry point below returns DSP_ERR_INVALID, nothing launched and nothing written, for: a NULL descriptor, profile, p_min or p_max;
 * B < 0 or above DSP_DAYS_MAX_PLANTS; days < 1 or above DSP_DAYS_MAX_DAYS; B * days above DSP_DAYS_MAX_POINTS; channels outside 1 .. 2;
 * filter outside 0 .. 1; channels == 2 with a NULL cf_series or start or N < 1; reserved != 0; K outside 1 .. DSP_DAYS_MAX_K; a NULL
 * array argument.  B == 0: DSP_OK, nothing launched.  All arrays are DEVICE arrays.  No allocation, no synchronisation.
 *
 * dsp_days_assign: one lane per point, plants fastest (the loads of one hour are consecutive); the centres [K][F] are staged once per
 * workgroup in LDS and read as a broadcast; the point stays in registers.  Writes label [days][B] and dist2 [days][B]. */
int dsp_days_assign(const dsp_days_desc *d, const double *centers, int32_t K, int32_t *label, double *dist2, void *hipStream);

/* dsp_days_update: the centres as the means of their members (labels >= 0; the others are skipped), the member counts and the inertia
 * = sum(dist2 of labelled points) / n_labelled (0 without a labelled point).  No floating-point atomics: the points of chunk q,
 * [q * DSP_DAYS_CHUNK, (q + 1) * DSP_DAYS_CHUNK), are added in the order of p into work[q][K * F + K + 2] (sums, counts, dist2, labelled points), then the
 * chunks in the order of q, and centre = sum / count - the same bits on every run.  A cluster without a member keeps its centre.
 * centers [K][F] in / out; count [K]; inertia [1]; work: at least dsp_days_work_doubles(B * days, K, channels) doubles.
 * Labels outside -2 .. K - 1 are the caller's fault and are skipped.  Two launches. */
int dsp_days_update(const dsp_days_desc *d, const int32_t *label, const double *dist2, int32_t K, double *centers, int64_t *count,
                    double *inertia, double *work, int64_t work_doubles, void *hipStream);
int64_t dsp_days_work_doubles(int64_t points, int32_t K, int32_t channels);      /* -1 for arguments outside their ranges            */

/* dsp_days_frequency: one lane per plant walks its `days` labels (Train_NN_Surrogates._generate_label_data).  filter == 1:
 * freq [B][K + 2] = [zero days, members of centre 0 .. K - 1, full days] / days;  filter == 0: freq [B][K] = members / days.  Counts are
 * integers, each entry one division.  No atomics. */
int dsp_days_frequency(const dsp_days_desc *d, const int32_t *label, int32_t K, double *freq, void *hipStream);

/* The scenario half of the Bidder's bid assembly ON THE DEVICE (reference: idaes Bidder._assemble_bids as DISPATCHES drives it -
 * dispatches/workflow/coordinator.py hands its bids to Prescient; golden values
 * dispatches/case_studies/renewables_case/tests/test_multiperiod_wind_battery_doubleloop.py:245-250): per hour t the pairs
 * (power[s][t], price[s][t]) of all scenarios, both numbers rounded to cents exactly as Python's round(v, 2) rounds them, pairs with
 * rounded power < p_min, non-finite numbers or ok[s] == 0 dropped, the highest price kept per distinct power, sorted by power.
 * One launch (one workgroup per hour: exact rounding, an LDS bitonic sort, an ordered compaction), no synchronisation.
 * power[s][t] = x[s][col[t][0]]                                                  (terms 0: the day-ahead power columns)
 *             = x[s][col[t][0]] * val[t][0] + constant[t]                        (terms 1)
 *             = (x[s][col[t][0]] * val[t][0] + x[s][col[t][1]] * val[t][1]) + constant[t]   (terms 2: P_T of the real-time models)
 * out[t][0] = number k of distinct powers of hour t, out[t][1 .. k] = the points: high 32 bits power cents, low 32 bits price cents
 * (both signed).  DSP_ERR_TOO_LARGE for B > DSP_BID_MAX_SCENARIOS or T > DSP_BID_MAX_HOURS (the caller keeps its own path then). */
#define DSP_BID_MAX_HOURS 64
#define DSP_BID_MAX_SCENARIOS 16384
typedef struct dsp_bid_request {
  int32_t B, T;                        /* scenarios, hours                                                                     */
  int32_t ldx, ldp;                    /* doubles per scenario in x / in price                                                 */
  int32_t terms;                       /* 0, 1 or 2 (above)                                                                    */
  int32_t reserved;
  const double *x;                     /* [B][ldx] DEVICE: the solution of the batch (dsp_batch::x of its solve)               */
  const double *price;                 /* [B][ldp] DEVICE: the energy prices the curve is built on, hour t in column t         */
  const uint8_t *ok;                   /* [B] DEVICE or NULL: 0 = the scenario offers nothing (not solved to optimality)       */
  int64_t *out;                        /* [T][B + 1] DEVICE                                                                    */
  double p_min;
  int32_t col[DSP_BID_MAX_HOURS][2];
  double val[DSP_BID_MAX_HOURS][2];
  double constant[DSP_BID_MAX_HOURS];
} dsp_bid_request;
int dsp_bid_points(const dsp_bid_request *rq, void *hipStream);

/* Stochastic mode of the wind + battery double loop ON THE DEVICE (ABI 13; dispatches_amd/rolling.py, n_price_scenarios / forecaster /
 * market): every plant b bids on S price scenarios - rows b * S + i of the bidding LPs' batches -, its (power, marginal price) pairs of
 * a period become ONE bid curve, and the market dispatches the plant along that curve at the price that occurs.
 *   scenario i with the backcast forecaster, hour-of-day `hod`, on simulated day d = hour / 24, period t:
 *     series[(start[b] + 24 (d - D) + (24 (D - 1 - i) + hod + t) mod (24 D)) mod N]      (workflow/forecaster.py: Backcaster._forecast
 *   over the D whole days before day d of the plant's own circular series); with the perfect forecaster: series[(start[b] + hour + t) mod N].
 *   curve of (plant, period): both numbers of every pair to integer cents exactly as Python's round(v, 2), pairs of rows whose solve is
 *   not optimal or with negative power dropped, the highest price per distinct power, the point (0, lowest price or 0) in front if no
 *   pair sits at power 0, running maximum over the prices: U_0 < U_1 < ..., M_0 <= M_1 <= ... (workflow/bid_curves.py with p_min = 0).
 *   clearing (workflow/market.py: clear_price_taker): dispatch = max{ U_j : M_j / 100 <= lmp }, U_0 if there is none; with the stub
 *   market the curve's last point. */
#define DSP_MARKET_MAX_T 48
#define DSP_MARKET_MAX_S 16
typedef struct dsp_market_model {
  double *c, *lb, *ub;                 /* [B * S][n] per-row vectors of a bidding LP (the dsp_batch inputs of its solves)          */
  const double *base_c;                /* [n] cost vector without prices                                                          */
  const double *x;                     /* [B * S][n] solution of its last solve                                                   */
  double *c0;                          /* [B * S] objective constant of every row or NULL                                         */
  const int32_t *status, *flags;       /* [B * S] outputs of its last solve (flags may be NULL)                                   */
  int32_t n, T;                        /* columns, horizon (T <= DSP_MARKET_MAX_T)                                                */
  int32_t soc_init, thr_init;          /* columns fixed to the realised state of charge / energy throughput                       */
  int32_t wind_cols[DSP_MARKET_MAX_T]; /* wind production column of every period (upper bound = availability)                     */
  int32_t pt_cols[DSP_MARKET_MAX_T][2];/* P_T[t] = 1e-3 (x[a] + x[b])                                                             */
  int32_t pda_cols[DSP_MARKET_MAX_T];  /* day-ahead power column of every period                                                  */
  double wind_kw, c0_base, waste_per_kw;
} dsp_market_model;

typedef struct dsp_market_state {
  int32_t B, S, D, N;                  /* plants, scenarios per plant (<= DSP_MARKET_MAX_S), history days, length of the series   */
  int32_t backcast, price_taker;       /* 0 / 1: forecaster (0 = perfect: S must be 1), market (0 = stub)                         */
  const int64_t *start;                /* [B] first hour of every plant's year in the series                                      */
  const int64_t *hour;                 /* [1] the clock (read only here)                                                          */
  const double *da_series, *rt_series, *cf_series;   /* [N]                                                                       */
  const double *soc, *thr;             /* [B] realised state                                                                      */
  const double *da_offer;              /* [B][24] cleared day-ahead dispatch of the current day (read by dsp_market_prepare, k >= 0)    */
  double *da_prices;                   /* [B][24] realised day-ahead prices of the current day (written by the day-ahead clearing)    */
  uint8_t *bad;                        /* [1] or NULL: set to 1 when a bidding solve left a status other than optimal             */
  int64_t *uncertified;                /* [1] or NULL: + the rows a solve left flagged DSP_FLAG_OBJ_WAIVED                        */
} dsp_market_state;

/* Scenario fan-out: objective, mutable bounds and objective constant of the B * S rows of bidding model `m` for the solve that follows.
 * k = -1: the day-ahead LP at hour 0 of the day (day_ahead_power free in every period); k = 0 .. 23: the real-time LP of hour-of-day k
 * (day-ahead prices and day_ahead_power of the periods inside the cleared day from da_prices / da_offer, as phase 0 of
 * dsp_wb_rolling_update).  One lane per row.  DSP_ERR_INVALID (nothing launched) for a NULL buffer, S or D out of range, a column
 * index outside [0, n). */
int dsp_market_prepare(const dsp_market_state *st, const dsp_market_model *m, int32_t k, void *hipStream);

/* Curve + clearing, one lane per (plant, period t < T): the S keys of the lane live in registers and are sorted by an unrolled
 * compare-exchange network.  Outputs: dispatch [B][T] MW, curve [B][T][S + 1][2] int32 cents (power, price; unused slots 0),
 * count [B][T] points of each curve.  Rows with status != 0 offer nothing and set dsp_market_state::bad.
 * k = -1 (day-ahead, T = 24): power = x[day_ahead_power column of t], prices = the day-ahead forecast, cleared at the realised
 *   day-ahead price; the realised prices go to da_prices (the loop passes its da_offer buffer as `dispatch`).
 * k = 0 .. 23 (real time, T <= 8): power = P_T[t], prices = the real-time forecast at hour-of-day k, cleared at the realised
 *   real-time price for t = 0 and at scenario 0's forecast for t >= 1.  With `tr` (the tracking model; may be NULL) the lane also
 *   does what phase 1 of dsp_wb_rolling_update does for the tracker: dispatch -> its dispatch rows, realised state, wind availability, c0. */
int dsp_market_clear(const dsp_market_state *st, const dsp_market_model *m, const dsp_wb_model *tr, int32_t k, int32_t T,
                     double *dispatch, int32_t *curve, int32_t *count, void *hipStream);

/* The same stochastic mode for ANY flowsheet of the reference, described instead of hard-coded (ABI 14; dispatches_amd/rolling_flowsheets.py:
 * BatchedDoubleLoop with n_price_scenarios / forecaster / market).  Scenarios, rows (b * S + i), curve and clearing rules are those of
 * dsp_market_* above, generalised three ways:
 *   power of a real-time pair   P_T[t] = (x[a] * pt_coef[t][0] + x[b] * pt_coef[t][1]) + pt_const[t]   (a term with column -1 is left out;
 *                               day-ahead pairs: x[pda_cols[t]]);
 *   minimum power               pairs whose rounded power is below p_min_cents are dropped and the point in front of a curve that has no
 *                               pair AT p_min_cents is (p_min_cents, lowest price or 0): Bidder._assemble_bids with the generator's
 *                               model_data.p_min (400 MW for the nuclear unit, 0 for the wind plants);
 *   state and wind              n_state <= 2 state columns fixed to state[b][j]; wind columns optional (wind_cols[0] = -1: none).
 * Objective of row r on its scenario's prices (every product rounded on its own, sums in the order of t):
 *   c[col] = base_c[col] - pt_coef * rt[t] on the P_T columns, c[pda_cols[t]] = base_c[..] - (da[t] - rt[t]),
 *   c0[r]  = (c0_base - sum_t rt[t] * pt_const[t]) + waste_per_kw * sum_t (wind availability of period t)    (last term with wind only). */
typedef struct dsp_loop_market_model {
  double *c, *lb, *ub;                 /* [B * S][n] per-row vectors of a bidding LP                                              */
  const double *base_c;                /* [n] cost vector without prices                                                          */
  const double *x;                     /* [B * S][n] solution of its last solve                                                   */
  double *c0;                          /* [B * S] objective constant of every row                                                 */
  const int32_t *status, *flags;       /* [B * S] outputs of its last solve (flags may be NULL)                                   */
  int32_t n, T, n_state;               /* columns, horizon (T <= DSP_MARKET_MAX_T), state columns (<= 2)                          */
  int32_t row_stride;                  /* (ABI 18; was reserved) doubles between two rows of c / lb / ub / x; 0 = n, as before, bit for
                                          bit.  A coupled self-schedule LP keeps its S scenario blocks of n columns side by side in
                                          one row: row_stride >= S * n, `n` and every column index describe ONE block.  Read by
                                          dsp_loop_schedule_prepare (all blocks) and dsp_loop_market_clear (x of block 0);
                                          dsp_loop_market_prepare takes 0 or n only.  status / flags / c0 stay one entry per row    */
  int32_t pt_cols[DSP_MARKET_MAX_T][2];/* -1 = no such term                                                                       */
  double  pt_coef[DSP_MARKET_MAX_T][2];
  double  pt_const[DSP_MARKET_MAX_T];
  int32_t pda_cols[DSP_MARKET_MAX_T];  /* day-ahead power column of every period                                                  */
  int32_t wind_cols[DSP_MARKET_MAX_T]; /* wind production column of every period; wind_cols[0] = -1: the flowsheet has no wind    */
  int32_t state_init[2];               /* columns fixed to the realised state                                                     */
  double wind_kw, c0_base, waste_per_kw;
  const double *wind_kw_plant, *c0_base_plant;       /* [B] per PLANT (not per row: row r reads plant r / S), both or neither
                                          (ABI 16, as dsp_loop_model): NULL = the scalars wind_kw / c0_base                       */
} dsp_loop_market_model;

typedef struct dsp_loop_market_state {
  int32_t B, S, D, N;                  /* as dsp_market_state                                                                     */
  int32_t backcast, price_taker;
  const int64_t *start;                /* [B]                                                                                     */
  const int64_t *hour;                 /* [1] the clock (read only here)                                                          */
  const double *da_series, *rt_series, *cf_series;   /* [N] (cf_series NULL without wind)                                         */
  const double *state;                 /* [B][n_state] realised state (NULL with n_state = 0)                                     */
  const double *da_offer;              /* [B][24] cleared day-ahead dispatch of the current day (read by prepare, k >= 0)         */
  double *da_prices;                   /* [B][24] realised day-ahead prices of the current day (written by the day-ahead clearing) */
  uint8_t *bad;                        /* [1] or NULL                                                                             */
  int64_t *uncertified;                /* [1] or NULL                                                                             */
  int64_t p_min_cents;                 /* minimum power of the generator in integer cents (>= 0)                                  */
  int32_t rt_history_lag_days;         /* (ABI 17) backcast only: the REAL-TIME scenarios come from a history that ends this many
                                          days earlier (0: as before, bit for bit; 1: a bid made at the RUC hour for the next day,
                                          when today is not a whole day of real-time prices yet).  >= 0, 24 (D + lag) <= N          */
  int32_t self_schedule;               /* (ABI 18; was reserved) dsp_loop_market_clear: 0 = as before, bit for bit; 1 = every pair is
                                          priced at 0 cents whatever the forecast (SelfScheduler._assemble_bids offers its schedule
                                          at cost 0): the curve is (p_min, 0), (schedule, 0)                                       */
  int32_t curve_slots;                 /* (ABI 18) points per stored curve in `curve`: 0 = S + 1, as before; otherwise
                                          S + 1 <= curve_slots <= DSP_MARKET_MAX_S + 1 (a loop that clears with an S = 1 state into
                                          buffers sized for its S price scenarios); unused slots are written 0                     */
  int32_t coupled;                     /* (ABI 19; was reserved) dsp_loop_market_clear: 0 = as before, bit for bit; 1 = the S scenarios
                                          of plant b are the S blocks of ONE coupled row (dsp_loop_monotone_prepare): x of scenario i
                                          at m->x + b * row_stride + i * n, status / flags one entry per plant at [b], a flagged
                                          plant counted once in `uncertified`.  Needs row_stride >= S * n and self_schedule = 0      */
  const int64_t *p_min_cents_plant;    /* (ABI 20) [B] DEVICE array or NULL: plant b's minimum power in integer cents where
                                          dsp_loop_market_clear reads p_min_cents (a nuclear plant's 500 MW - its PEM size).  NULL = the
                                          scalar, ABI 19 bit for bit.  Every entry is bounded like the scalar, 0 .. 2e9: the host
                                          reads the array back and refuses (DSP_ERR_INVALID, nothing written) an entry outside -
                                          unless hipStream is being captured, when it cannot read: capture after an eager call     */
} dsp_loop_market_state;

/* Scenario fan-out of bidding model `m` (B * S rows), one lane per row.  k = -1: the day-ahead LP (day_ahead_power free in every period);
 * k = 0 .. 23: the real-time LP of hour-of-day k (day-ahead prices and day_ahead_power of the min(T, 24 - k) periods inside the cleared
 * day from da_prices / da_offer).  DSP_ERR_INVALID, nothing launched and nothing written, for: a NULL buffer that is used; S, D, T,
 * n_state or k out of range; a used column index outside [0, n); n_state > 0 with a NULL state; wind columns with a NULL cf_series. */
int dsp_loop_market_prepare(const dsp_loop_market_state *st, const dsp_loop_market_model *m, int32_t k, void *hipStream);

/* Curve + clearing, one lane per (plant, period t < T), keys in registers as dsp_market_clear.  Outputs as dsp_market_clear: dispatch
 * [B][T] MW, curve [B][T][S + 1][2] int32 cents, count [B][T]; status / flags of the bidding solve are folded into bad / uncertified.
 * k = -1 (T <= 24): day-ahead pairs, cleared at the realised day-ahead price, which goes to da_prices; `tr` must be NULL.
 * k = 0 .. 23 (T <= DSP_LOOP_MAX_T): real-time pairs, cleared at the realised price (t = 0) / scenario 0's forecast (t >= 1).  With `tr`
 * (the tracking model of B rows, tr->T == T) the lanes also write the tracker's LP of this hour: dispatch rows = dispatch[t] -
 * tr->pt_const[t], state columns, wind availability and c0 = c0_base + waste_per_kw * sum_t availability (as phase 1 of dsp_loop_update).
 * Refusals as dsp_loop_market_prepare, and for a dispatch row of `tr` outside [0, tr->m).
 * ABI 18: x of row r is read at m->x + r * (row_stride ? row_stride : n) - with an S = 1 state and the descriptor of
 * dsp_loop_schedule_prepare that is block 0 of plant r's coupled row, the schedule; st->self_schedule prices every pair at 0 cents and
 * st->curve_slots sets the stride of `curve`.  All three are kernel arguments, uniform over the grid; 0 / 0 / 0 is ABI 17 bit for bit.
 * Refused: 0 < row_stride < n, curve_slots outside {0} and S + 1 .. DSP_MARKET_MAX_S + 1, self_schedule outside 0 / 1.
 * ABI 19: st->coupled = 1 reads the S pairs of plant b and period t from the S blocks of plant b's ONE coupled row (x at
 * m->x + b * row_stride + i * n, priced at scenario i's forecast as before); status[b] / flags[b] of the plant's one solve stand for all
 * its S pairs and a flagged plant is counted once.  A kernel argument, uniform over the grid; 0 is ABI 18 bit for bit.  Refused (by
 * every dsp_loop_market_* entry point): coupled outside 0 / 1, coupled with self_schedule = 1; by the clearing: coupled with
 * row_stride < S * n.
 * Per-plant sizes (ABI 16; BatchedDoubleLoop(wind_mw=, battery_mw=, battery_mwh=)): with wind_kw_plant / c0_base_plant the lanes read
 * plant b's wind capacity and objective constant at the very sites that read the scalars - same intrinsics, same order, so that kernel
 * = tensor form = graph replay stays bit for bit.  A size is never a matrix coefficient of these flowsheets: the battery's power and
 * energy limits are static column / row bounds that the caller writes once into lb / ub / rhi.  DSP_ERR_INVALID, nothing launched, for
 * one of the two pointers without the other, for per-plant pointers on a model without wind columns, and for `m` and `tr`
 * (dsp_loop_update: `rt` and `tr`) that do not carry them together. */
int dsp_loop_market_clear(const dsp_loop_market_state *st, const dsp_loop_market_model *m, const dsp_loop_model *tr, int32_t k, int32_t T,
                          double *dispatch, int32_t *curve, int32_t *count, void *hipStream);

/* The day-ahead LP of a SELF-SCHEDULING plant (ABI 18; dispatches_amd/rolling_flowsheets.py: BatchedDoubleLoop with
 * bidder="self_schedule").  The reference's run_double_loop_battery.py --participation_mode SelfSchedule bids with idaes' SelfScheduler,
 * which ties the S price scenarios of the day-ahead problem to ONE schedule, day_ahead_power[s, t] == day_ahead_power[0, t]
 * (workflow/coupling.py::CoupledScenarioModel, "non_anticipative").  That is one LP per plant: S blocks of the scenario LP side by side in
 * a row of m->row_stride >= S * m->n doubles, plus (S - 1) T static coupling rows that the caller writes once (bounds 0, 0).
 * `m` describes ONE block: n, pt_cols, pda_cols, wind_cols and state_init are relative to the block; c / lb / ub are [B][row_stride],
 * c0 is [B].  One lane per (plant b, scenario i) writes block i of row b exactly as dsp_loop_market_prepare with k = -1 writes row
 * b * S + i: objective on scenario i's backcast prices (same index rule, products rounded on their own), state columns, wind bounds,
 * day_ahead_power free in every period.  The lane of scenario 0 also writes the row's constant
 *   c0[b] = sum_i ((c0_base - sum_t rt_i[t] * pt_const[t]) + waste_per_kw * sum_t availability[t]),   accumulated in the order of i
 * (inner sums in the order of t): one lane, no atomics - bit-identical to the tensor form.
 * DSP_ERR_INVALID, nothing launched and nothing written, for: what dsp_loop_market_prepare refuses (a NULL buffer that is used; S, D, T
 * or n_state out of range; a used column index outside the block [0, n); n_state > 0 with a NULL state; wind columns with a NULL
 * cf_series); row_stride < S * n; per-plant size pointers (a self-scheduling batch has one plant size). */
int dsp_loop_schedule_prepare(const dsp_loop_market_state *st, const dsp_loop_market_model *m, void *hipStream);

/* The day-ahead LP of a plant whose BID CURVE IS MONOTONE across its price scenarios (ABI 19; dispatches_amd/rolling_flowsheets.py:
 * BatchedDoubleLoop with bidder="lp", scenario_coupling="monotone").  idaes' Bidder ties every pair of scenarios j < k in every period,
 *   (day_ahead_power[k, t] - day_ahead_power[j, t]) * (price[k, t] - price[j, t]) >= 0
 * (workflow/coupling.py::CoupledScenarioModel, "monotone").  That is one LP per plant: the S blocks of dsp_loop_schedule_prepare - `m`
 * describes ONE block, row_stride >= S * n, c0 is [B] - plus P T rows pda[k, t] - pda[j, t], P = S (S - 1) / 2, pairs in the order
 * (0, 1) .. (0, S - 1), (1, 2) .. (k fastest), row first_coupling_row + p * T + t.  Their coefficients are static; their BOUNDS follow
 * the order of plant b's day-ahead scenario prices (the index rule of the blocks' objective): with d = da[k, t] - da[j, t],
 *   rlo = 0 if d > 0 else -inf,   rhi = 0 if d < 0 else +inf.
 * rlo / rhi are the coupled model's row-bound buffers [B][m_rows]; only the P T rows from first_coupling_row on are written.
 * One launch over two lane ranges: lanes [0, B * S) write the blocks and c0[b] exactly as dsp_loop_schedule_prepare does, the next
 * B * P * T lanes one (b, p, t) each, t fastest.  No atomics; bit-identical to the tensor form.
 * DSP_ERR_INVALID, nothing launched and nothing written, for: everything dsp_loop_schedule_prepare refuses; NULL rlo / rhi; S < 2 (no
 * pairs); first_coupling_row < 0; first_coupling_row + P * T > m_rows. */
int dsp_loop_monotone_prepare(const dsp_loop_market_state *st, const dsp_loop_market_model *m, double *rlo, double *rhi, int32_t m_rows,
                              int32_t first_coupling_row, void *hipStream);

/* The coupled REAL-TIME LP of a look-ahead hour past midnight (added under ABI 22; BatchedDoubleLoop with past_midnight="coupled").  In
 * the last T - 1 hours of a day (24 - k < T) the real-time problem of hour k has periods past midnight whose day_ahead_power is free, and
 * the host bidders tie those across the price scenarios (workflow/bidder.py::compute_real_time_bids on CoupledScenarioModel).  `m`
 * describes ONE block of a coupled row as for dsp_loop_schedule_prepare (row_stride >= S * n, c0 is [B]).  Lane (b, i) writes block i of
 * row b exactly as dsp_loop_market_prepare writes row b * S + i at hour k - scenario i's backcast prices asked at hour-of-day k, the
 * realised day-ahead prices and the cleared day_ahead_power in the 24 - k periods inside the day, day_ahead_power on (0, inf) past
 * midnight, plant b's state and wind - and the lane of scenario 0 writes c0[b], the S block constants added in the order of i.
 * rlo / rhi != NULL (the monotone Bidder): the next B * P * T lanes, P = S (S - 1) / 2, write the bounds of the ordered-pair rows
 * first_coupling_row + p * T + t of ALL T periods from the order of the hour's REAL-TIME scenario prices (through rt_history_lag_days):
 *   d = rt[k', t] - rt[j, t],   rlo = 0 if d > 0 else -inf,   rhi = 0 if d < 0 else +inf,
 * pairs and lane order as dsp_loop_monotone_prepare.  rlo == rhi == NULL: a self-schedule, whose coupling rows are static (0, 0).
 * No atomics, no cross-lane traffic; bit-identical to the tensor form (BatchedDoubleLoop._tied_blocks).  dsp_loop_market_clear reads such
 * a row with k >= 0 as it reads the day-ahead one (coupled = 1, or block 0 through row_stride).
 * DSP_ERR_INVALID, nothing launched and nothing written, for: everything dsp_loop_schedule_prepare refuses; k outside 0 .. 23 or an hour
 * whose horizon stays inside the day (24 - k >= T); a NULL da_offer / da_prices; one of rlo / rhi NULL and the other not; with rlo / rhi:
 * S < 2, first_coupling_row < 0, first_coupling_row + P * T > m_rows.
 * Capturable: one kernel launch on hipStream, no allocation, no synchronisation, no memset. */
int dsp_loop_midnight_prepare(const dsp_loop_market_state *st, const dsp_loop_market_model *m, double *rlo, double *rhi, int32_t m_rows,
                              int32_t first_coupling_row, int32_t k, void *hipStream);

/* Parametrized two-tier bidding in the descriptor loop (ABI 15; dispatches_amd/rolling_flowsheets.py: BatchedDoubleLoop with
 * bidder="parametrized").  The reference's wind + PEM and wind + battery sweeps bid without an LP (PEM_parametrized_bidder.py:50-122,
 * battery_parametrized_bidder.py:47-123): with w = wind_mw * capacity factor of the period, the pairs of a (plant, period) are
 *   (0, 0), (max(0, w - storage_mw[b]), 0), (p_max, bid_price[b]),   p_max = w (wind + PEM) or max(w, storage_mw[b]) (battery != 0).
 * They become a curve by the rules of dsp_loop_market_clear with S = 3 and p_min = 0 (integer cents, the highest price per distinct
 * power, running maximum: 1 .. 3 points in a slot of 4) and are cleared the same way (price taker: the last point whose price the LMP
 * covers; stub: the last point).  Three pairs need no sort: the curve is a closed form of the three cent values.
 * bid_price and storage_mw must be finite and >= 0, the series finite, start[b] in [0, N): device data, not checked by the entry point. */
typedef struct dsp_loop_param_state {
  int32_t B, N;                        /* plants (>= 1), length of the series (>= 24)                                             */
  int32_t price_taker, battery;        /* 0 / 1: market (0 = stub), p_max rule (1 = max(w, storage_mw): wind + battery)           */
  const int64_t *start;                /* [B] first hour of every plant's year (several plants may share one)                     */
  const int64_t *hour;                 /* [1] the clock (read only here)                                                          */
  const double *da_series, *rt_series; /* [N] day-ahead / real-time prices                                                        */
  const double *da_cf_series, *rt_cf_series;         /* [N] day-ahead / real-time capacity factors                                */
  const double *state;                 /* [B][n_state] realised state (NULL with n_state = 0)                                     */
  const double *bid_price, *storage_mw;              /* [B] the two parameters of every plant                                     */
  double wind_mw;                      /* w = wind_mw * capacity factor                                                           */
  double *da_offer, *da_prices;        /* [B][24] written by phase 0                                                              */
  int32_t *da_curve, *da_count;        /* [B][24][4][2] cents (power, price; unused slots 0), [B][24]                             */
  double *rt_dispatch;                 /* [B][T] written by phase 1                                                               */
  int32_t *rt_curve, *rt_count;        /* [B][T][4][2], [B][T]                                                                    */
  double *h2_kg;                       /* [B] or NULL (no electrolyser): += ((x[pem_col] * h2_mul) / h2_div) * 3600 in phase 2    */
  double h2_mul, h2_div;
  int32_t pem_col, reserved;           /* column of the tracker holding the first period's PEM electricity                        */
} dsp_loop_param_state;

/* phase 0 (k = -1), one lane per (plant, hour of 24): day-ahead curves on da_cf_series, cleared at the realised day-ahead price ->
 *          da_offer, da_prices, da_curve, da_count.  `tr` is not touched (only tr->T is checked).
 * phase 1 (k = 0 .. 23), one lane per (plant, period t < tr->T): real-time curves on rt_cf_series, cleared at the real-time price of
 *          period t -> rt_dispatch, rt_curve, rt_count; the tracker's LP of this hour as dsp_loop_market_clear writes it (dispatch
 *          rows = dispatch - tr->pt_const[t]; by the lane of period 0: state columns, wind upper bounds, c0).
 * phase 2 (k = 0 .. 23), one lane per plant, after the tracking solve: the hydrogen of the implemented hour -> h2_kg.  Hand-off,
 *          revenue and clock stay with phase 2 of dsp_loop_update.
 * DSP_ERR_INVALID, nothing launched and nothing written, for: B < 1; N < 24; tr->T outside 1 .. DSP_LOOP_MAX_T; a NULL series, start,
 * hour, parameter array or output of the phase; phase 1: a dispatch row outside [0, tr->m), a wind column (when wind_cols[0] >= 0) or a
 * state column outside [0, tr->n), n_state outside 0 .. 2 or > 0 with a NULL state, NULL rlo / rhi / lb / ub / c0; phase 2: NULL
 * h2_kg or tr->x, pem_col outside [0, tr->n); a phase outside 0 .. 2 or a k that does not belong to it. */
int dsp_loop_param_step(const dsp_loop_param_state *st, const dsp_loop_model *tr, int32_t phase, int32_t k, void *hipStream);

/* Day-ahead bidding at the RUC hour on a PROJECTED state (ABI 17; dispatches_amd/rolling_flowsheets.py: BatchedDoubleLoop with
 * ruc_hour=H, 1 <= H <= 23).  In the reference the day-ahead market of day d + 1 runs at hour H of day d: the coordinator clones the
 * tracker into a projection tracker, tracks the not yet delivered part of today's cleared day-ahead dispatch to midnight and hands the
 * projected state to the day-ahead bidder (DoubleLoopCoordinator.bid_into_DAM; workflow/coordinator.py::_project_tracking_trajectory).
 * `pj` is that projection tracker: a dsp_loop_model of its own (own buffers, own solver handle) on the tracker's template.
 * Chain step j = 0 .. 24 - H - 1, at loop clock *hour = 24 d + H:
 *   phase 0 (write, before the solve), one lane per (plant, period t < pj->T):
 *            dispatch row t = da_offer[b][H + j + t] - pj->pt_const[t] where H + j + t < 24, free on both sides (-inf, +inf) past
 *            midnight; by the lane of period 0: state columns = state[b] (j = 0, also copied to proj_state[0]) or proj_state[j][b],
 *            wind upper bounds of the window that starts at clock + j, c0 = c0_base + waste_per_kw * sum_t availability (the tracker
 *            half of dsp_loop_market_clear, per-plant sizes included).
 *   phase 1 (hand-off, after the solve), one lane per plant: status / flags -> bad / uncertified; proj_real[j][b] = x[state_real];
 *            proj_state[j + 1][b] = rint(x[state_real] * state_scale) / state_scale; proj_obj[j][b] = obj[b] + c0[b].
 *   phase 2 (activate, midnight; j = 0; pj is not touched and may be NULL), one lane per (plant, hour of 24): pend_offer ->
 *            da_offer, pend_prices -> da_prices and, with slots > 0, pend_curve / pend_count -> da_curve / da_count.
 * DSP_ERR_INVALID, nothing launched and nothing written, for: B < 1; N < 1; ruc_hour outside 1 .. 23; a phase outside 0 .. 2; j outside
 * 0 .. 24 - ruc_hour - 1 (phase 2: j != 0); a NULL pointer the phase uses; phases 0 / 1: pj->T outside 1 .. DSP_LOOP_MAX_T, n_state
 * outside 0 .. 2, a dispatch row outside [0, pj->m), a wind, state_init or state_real column outside [0, pj->n), wind columns with a
 * NULL cf_series, one per-plant pointer without the other or without wind columns; phase 2: slots < 0 or > DSP_MARKET_MAX_S + 1. */
typedef struct dsp_loop_project_state {
  int32_t B, N;
  int32_t ruc_hour;                    /* H: hour of the day at which the chain starts                                            */
  int32_t slots;                       /* points per stored curve (S + 1); 0 = the loop keeps no curves (deterministic mode)      */
  const int64_t *start;                /* [B]                                                                                     */
  const int64_t *hour;                 /* [1] the loop's clock (read only here)                                                   */
  const double *cf_series;             /* [N] or NULL without wind                                                                */
  const double *state;                 /* [B][n_state] realised state (NULL with n_state = 0)                                     */
  double state_scale[2];
  const double *obj;                   /* [B] objective of pj's last solve, without its constant                                  */
  double *proj_state;                  /* [24 - H + 1][B][n_state] the trace: entry 0 realised, the last one what the bid uses    */
  double *proj_real;                   /* [24 - H][B][n_state] unrounded                                                          */
  double *proj_obj;                    /* [24 - H][B] objective including c0                                                      */
  uint8_t *bad;                        /* as dsp_loop_state                                                                       */
  int64_t *uncertified;
  double *da_offer, *da_prices;        /* [B][24] current day: da_offer read by phase 0, both written by phase 2                  */
  const double *pend_offer, *pend_prices;            /* [B][24] the bid made at the RUC hour for the next day                     */
  int32_t *da_curve, *da_count;        /* [B][24][slots][2], [B][24] (slots > 0)                                                  */
  const int32_t *pend_curve, *pend_count;
} dsp_loop_project_state;
int dsp_loop_project(const dsp_loop_project_state *st, const dsp_loop_model *pj, int32_t phase, int32_t j, void *hipStream);

/* Introspection */
int dsp_get_dims(const dsp_handle *h, int32_t *n, int32_t *m, int64_t *nnz);
/* run-time specialisation (dsp_options::no_rtc): compile one shape without a GPU (returns the code size, 0 + reason in msg);
 * why a handle runs on an ahead-of-time kernel instead ("" if it was specialised) */
int dsp_rtc_compile_check(int cpl, int rpl, int has_long, unsigned wc_pack, unsigned wr_pack, int qp, char *msg, int msg_len);
const char *dsp_rtc_message(const dsp_handle *h);
int dsp_get_scaling(const dsp_handle *h, double *row_scale /*[m]*/, double *col_scale /*[n]*/, double *step_eta);

int dsp_destroy(dsp_handle *h);
const char *dsp_strerror(int code);
int dsp_last_hip_error(void);
int dsp_version(void);
/* The first 16 hex digits of the SHA-256 over the library's sources (csrc/ *.hip, *.hpp and this header, in name order, each preceded
 * by its base name) as they were when it was compiled ("unknown" for a build that did not pass -DDSP_SOURCE_HASH).  A binding that sits next to the sources compares it with the files it sees and refuses a stale binary
 * (dispatches_amd/hip_solver.py::load_library); bench.py prints it, so that a measured number names the code that produced it. */
const char *dsp_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* DSP_HIP_H */
