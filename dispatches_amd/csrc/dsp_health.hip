// dsp_health.hip — the per-plant solve health of the descriptor double loop on the device, gfx950 only (include/dsp_hip.h:
// dsp_loop_health, added under ABI 22; rolling_flowsheets.py::BatchedDoubleLoop(health=True)).
//
// The loop's two global flags - `bad`, one bool, and `uncertified`, one count - say that SOME row of SOME plant failed or was accepted
// without a certified objective.  This kernel keeps the same facts per plant and per kind of solve (day-ahead, real-time, tracking,
// projection), and what the solves cost: after every solve of a step, one launch reads the solve's status / flags / iters and books the
// R = rows_per_plant consecutive rows b * R .. b * R + R - 1 to plant b.
//
//   loop_health_kernel   one lane per plant.  The lane reads the clock once, walks its R <= 16 rows in the order of i, and updates its own
//                        seven entries - solves, fail, status_mask, waived, iters, iters_max of (kind, b) and first[b] - with plain
//                        vector loads and stores.  No atomics (a plant's entries belong to one lane), no LDS, no cross-lane traffic,
//                        integer arithmetic only: the tensor form (BatchedDoubleLoop._health_book, use_fused=False) is equal exactly.
//
// Nothing here writes `bad` / `uncertified`: those stay with the kernels that fold the same rows (dsp_loop.hip, dsp_market.hip,
// dsp_project.hip), and the two pairs are tested against each other.  The host entry point checks every pointer and size, so that a lane
// never indexes outside [0, B * R) of the solve's arrays or [0, 4 * B) of the counters.  VGPRs / scratch:
// profiles/loop_device_kernel_resources.txt.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dsp_hip.h"
#include "dsp_capi_internal.hpp"

static_assert(sizeof(dsp_loop_health_state) + 64 <= 4096, "the descriptor travels as a by-value kernel argument: HIP's limit is 4 KB");

__global__ void __launch_bounds__(256) loop_health_kernel(dsp_loop_health_state h, const int32_t *status, const int32_t *flags,
                                                          const int32_t *iters, int R, int kind) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= h.B) return;
  const long long clock = *h.clock;
  const size_t row0 = (size_t)b * (size_t)R, at = (size_t)kind * (size_t)h.B + (size_t)b;
  int fail = 0, mask = 0, waived = 0, most = 0;
  long long sum = 0;
  for (int i = 0; i < R; ++i) {
    const int s = status[row0 + i];
    if (s != 0) {
      ++fail;
      mask |= 1 << ((s >= 1 && s <= 29) ? s : 30);
    } else if (flags && (flags[row0 + i] & DSP_FLAG_OBJ_WAIVED)) {
      ++waived;
    }
    if (iters) {
      const int it = iters[row0 + i];
      sum += it;
      most = it > most ? it : most;
    }
  }
  h.solves[at] += R;
  h.fail[at] += fail;
  h.status_mask[at] |= mask;
  if (flags) h.waived[at] += waived;
  if (iters) {
    h.iters[at] += sum;
    const int before = h.iters_max[at];
    h.iters_max[at] = most > before ? most : before;
  }
  if (fail != 0 && h.first[b] == 0) h.first[b] = clock + 1;
}

extern "C" int dsp_loop_health(const dsp_loop_health_state *h, const int32_t *status, const int32_t *flags, const int32_t *iters,
                               int32_t rows_per_plant, int32_t kind, void *hipStream) {
  if (!h || !status || h->B < 1 || h->reserved != 0) return DSP_ERR_INVALID;
  if (rows_per_plant < 1 || rows_per_plant > DSP_HEALTH_MAX_ROWS || kind < 0 || kind >= DSP_HEALTH_KINDS) return DSP_ERR_INVALID;
  if (!h->clock || !h->solves || !h->fail || !h->status_mask || !h->waived || !h->iters || !h->iters_max || !h->first) return DSP_ERR_INVALID;
  hipLaunchKernelGGL(loop_health_kernel, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, (hipStream_t)hipStream, *h, status, flags, iters,
                     (int)rows_per_plant, (int)kind);
  HIP_TRY(hipGetLastError());
  return DSP_OK;
}
