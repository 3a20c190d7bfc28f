// dsp_project.hip — the projection tracker of the descriptor double loop on the device, gfx950 only (include/dsp_hip.h:
// dsp_loop_project; rolling_flowsheets.py: BatchedDoubleLoop with ruc_hour=H).
//
// Reference behaviour (DoubleLoopCoordinator.bid_into_DAM as run_double_loop_battery.py:255-294 drives it; the project's restatement is
// workflow/coordinator.py::_project_tracking_trajectory): the day-ahead market of day d + 1 runs at hour H of day d.  A clone of the
// tracker follows the part of today's cleared day-ahead dispatch that is not delivered yet, hour by hour to midnight, and the state it
// ends in - not a realised one - is what the day-ahead bid of day d + 1 starts from.  24 - H dependent tracking solves per day, each
// between two launches of this file:
//
//   project_write_kernel     one lane per (plant, period) of chain step j: dispatch row t = da_offer[H + j + t] - pt_const[t] inside the
//                            day, FREE ON BOTH SIDES (-inf, +inf) past midnight (Tracker._pass_market_dispatch on a short dispatch
//                            list); by the lane of period 0 the state columns (step 0: the realised state, which becomes entry 0 of the
//                            trace; step j: entry j), the wind bounds of the window at clock + j and c0 (loop_tracker_plant,
//                            dsp_loop_device.hpp: the plant half of every descriptor tracker's LP).
//   project_hand_off_kernel  one lane per plant after the solve: status / flags -> bad / uncertified, the unrounded state -> proj_real[j],
//                            rounded as update_model rounds it -> proj_state[j + 1], objective with its constant -> proj_obj[j].
//   project_activate_kernel  midnight, one lane per (plant, hour of 24): the pending bid (offers, realised day-ahead prices, curves,
//                            counts) becomes the current one.
//
// Arithmetic of dsp_loop_device.hpp: every product rounded on its own and opaque before a sum takes it, sums in the order of
// t - bit-identical to the tensor operations of BatchedDoubleLoop (use_fused=False).  Vector stores only, no LDS, no atomics beyond the
// `uncertified` counter of the other loop kernels; VGPRs / scratch: profiles/loop_device_kernel_resources.txt.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dsp_hip.h"
#include "dsp_device.hpp"
#include "dsp_loop_device.hpp"

#pragma clang fp contract(off)

namespace dsp {

static_assert(sizeof(dsp_loop_project_state) + sizeof(dsp_loop_model) + 64 <= 4096,
              "the descriptors travel as by-value kernel arguments: HIP's limit is 4 KB");

__global__ void __launch_bounds__(256) project_write_kernel(dsp_loop_project_state s, dsp_loop_model pj, int j) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= s.B * pj.T) return;
  const int b = g / pj.T, t = g - b * pj.T;
  const int at = s.ruc_hour + j + t;                                 // hour of the day this period tracks
  double *rlo = pj.rlo + (size_t)b * pj.m, *rhi = pj.rhi + (size_t)b * pj.m;
  if (at < 24) {
    const double rhs = __dsub_rn(s.da_offer[(size_t)b * 24 + at], pj.pt_const[t]);
    rlo[pj.track_rows[t]] = rhs;
    rhi[pj.track_rows[t]] = rhs;
  } else {                                                           // past midnight: no dispatch yet, the row is free on both sides
    rlo[pj.track_rows[t]] = -INFINITY;
    rhi[pj.track_rows[t]] = INFINITY;
  }
  if (t != 0) return;
  const double *state = s.proj_state + ((size_t)j * s.B + b) * pj.n_state;     // entry j of the trace
  if (j == 0) {                                                      // entry 0: the realised state at the bid hour
    state = s.state + (size_t)b * pj.n_state;
    for (int e = 0; e < pj.n_state; ++e) s.proj_state[(size_t)b * pj.n_state + e] = state[e];
  }
  loop_tracker_plant(pj, b, s.cf_series, s.start[b] + *s.hour + j, s.N, state);
}

__global__ void __launch_bounds__(256) project_hand_off_kernel(dsp_loop_project_state s, dsp_loop_model pj, int j) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= s.B) return;
  if (pj.status[b] != 0 && s.bad) *s.bad = 1;
  if (pj.flags && s.uncertified && (pj.flags[b] & DSP_FLAG_OBJ_WAIVED)) atomicAdd(reinterpret_cast<unsigned long long *>(s.uncertified), 1ull);
  const double *x = pj.x + (size_t)b * pj.n;
  const size_t plane = (size_t)s.B * pj.n_state;
  for (int e = 0; e < pj.n_state; ++e) {
    const size_t at_state = (size_t)b * pj.n_state + e;
    const double real = x[pj.state_real[e]];
    s.proj_real[(size_t)j * plane + at_state] = real;
    s.proj_state[(size_t)(j + 1) * plane + at_state] = __ddiv_rn(rint(loop_opaque(__dmul_rn(real, s.state_scale[e]))), s.state_scale[e]);
  }
  s.proj_obj[(size_t)j * s.B + b] = __dadd_rn(s.obj[b], pj.c0[b]);
}

__global__ void __launch_bounds__(256) project_activate_kernel(dsp_loop_project_state s) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= s.B * 24) return;
  s.da_offer[g] = s.pend_offer[g];
  s.da_prices[g] = s.pend_prices[g];
  if (s.slots > 0) {
    s.da_count[g] = s.pend_count[g];
    const size_t base = (size_t)g * s.slots * 2;
    for (int q = 0; q < 2 * s.slots; ++q) s.da_curve[base + q] = s.pend_curve[base + q];
  }
}

hipError_t launch_loop_project(const dsp_loop_project_state &st, const dsp_loop_model &pj, int phase, int j, hipStream_t stream) {
  const dim3 block(256);
  if (phase == 0) {
    const long long lanes = (long long)st.B * pj.T;
    hipLaunchKernelGGL(project_write_kernel, dim3((unsigned)((lanes + 255) / 256)), block, 0, stream, st, pj, j);
  } else if (phase == 1) {
    hipLaunchKernelGGL(project_hand_off_kernel, dim3((unsigned)((st.B + 255) / 256)), block, 0, stream, st, pj, j);
  } else {
    const long long lanes = (long long)st.B * 24;
    hipLaunchKernelGGL(project_activate_kernel, dim3((unsigned)((lanes + 255) / 256)), block, 0, stream, st);
  }
  return hipGetLastError();
}

}  // namespace dsp
