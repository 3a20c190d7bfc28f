// dsp_kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the batched dispatch-LP solver.
//
// Hot path: one price scenario per 64-lane wave (pdlp_solve_kernel).
//   * lane l owns CPL columns and RPL rows; every per-scenario vector (x, anchor, c, bounds, y, anchor, row bounds)
//     lives in that lane's registers for the whole solve; lanes exchange x-bar / y through a per-wave LDS buffer (one
//     ds_write_b64 per owned element, one ds_read_b64 gather per matrix entry, slots permuted against bank conflicts);
//   * the scaled constraint matrix, shared by all scenarios, is held in one of two forms:
//       - register-resident (RegEll; every LP of the reference workflows): each lane keeps the entries of the vectors
//         it owns in VGPRs, pre-multiplied by the step sizes (tau A^T and -sig A), so a PDHG half-step is a chain of
//         FMAs that starts from x - tau c / y; ownership is sorted by vector length and the ELL width is per slot;
//       - LDS-resident (any other LP that fits): staged once per workgroup as 16-byte {value, byte offset} entries in a
//         lane-major ELL layout, one conflict-free ds_read_b128 per entry;
//   * vectors longer than the ELL width (e.g. the shared PEM-capacity column) are reduced cooperatively by the wave;
//   * the iteration is the restarted, reflected Halpern PDHG (r2HPDHG): two SpMVs per iteration, NO reduction on the
//     per-iteration path; every `check_every` iterations one extra SpMV + one wave reduction give the fixed-point
//     residual for the restart test; the KKT / termination test is scheduled from that residual (dsp_options::kkt_gate);
//   * "ray jumps": PDHG on an LP is piecewise affine; while the active set is not yet identified the iterates drift
//     along a ray z + k v at constant speed for thousands of iterations.  When the check detects such a steady
//     state (T(T z) - T z == T z - z), a ratio test over all clipping thresholds (one wave-min) gives the number of
//     steps to the next breakpoint and the iterate jumps there in one go;
//   * scenarios are pulled from a device-side work queue (one atomicAdd per scenario) so waves retire
//     independently — iteration counts differ 20-fold between price scenarios.
// Control flow is wave-uniform throughout (one scenario per wave): no divergence.  Wave reductions run on the VALU (DPP).
// No MFMA: the work is sparse BLAS-2 with ~3 nonzeros per row.  HBM is touched only to load a scenario's
// (c, bounds) and to store (x, y, obj); FP64 VALU issue and the LDS pipe limit it about equally.
//
// The streaming SpMV step kernel at the bottom keeps X/Y in HBM and is the kernel whose HBM roofline
// SURVEY.md 8(d) defines.
#ifdef __HIPCC_RTC__     /* run-time compilation (hiprtc, dsp_rtc.cpp): no system headers, the HIP device API is built in */
#ifndef DSP_RTC_TYPES
#define DSP_RTC_TYPES
typedef signed char int8_t; typedef unsigned char uint8_t; typedef short int16_t; typedef unsigned short uint16_t;
typedef int int32_t; typedef unsigned int uint32_t; typedef long long int64_t; typedef unsigned long long uint64_t;
typedef unsigned long uintptr_t; typedef unsigned long size_t;
#ifndef INFINITY
#define INFINITY (__builtin_inff())
#endif
#ifndef NAN
#define NAN (__builtin_nanf(""))
#endif
#endif
#else
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#endif

#include "dsp_device.hpp"
#include "dsp_wave.hpp"

namespace dsp {

// DSP_LEGACY_PULL (development): the round-1 form of the work-queue pull, kept to reproduce the hang it caused - see
// the comment at the pull.
#ifdef DSP_DEBUG_TRACE
#define DSP_TRACE(...) do { if (threadIdx.x == 0 && blockIdx.x == 0) printf(__VA_ARGS__); } while (0)
#else
#define DSP_TRACE(...) do { } while (0)
#endif

// steps until the clipped quantity g (moving by dg per step) changes its class among {< lo, [lo, hi], > hi}
__device__ __forceinline__ double steps_to_break(double g, double dg, double lo, double hi) {
  double a = INFINITY;
  if (dg > 0.0) {
    if (g < lo) a = (lo - g) / dg;
    else if (g <= hi) a = (hi - g) / dg;
  } else if (dg < 0.0) {
    if (g > hi) a = (hi - g) / dg;
    else if (g >= lo) a = (lo - g) / dg;
  }
  return (a == a) ? a : INFINITY;
}

// ---- lane-major ELL products --------------------------------------------------------------------------------
// out[q] = sum_e ell[(e*S+q)*64+lane].v * vec[ell[...].off]   for the S slots this lane owns, + long vectors.
template <int S, bool LONG>
__device__ __forceinline__ void ell_product(double (&out)[S], const Entry *__restrict__ ell, int W,
                                            const char *vec /* per-wave LDS exchange buffer */, int lane,
                                            const LongList &ll, const Entry *__restrict__ tail) {
#pragma unroll
  for (int q = 0; q < S; ++q) out[q] = 0.0;
  const int4 *p = reinterpret_cast<const int4 *>(ell + lane);
#pragma unroll 1
  for (int e = 0; e < W; ++e, p += S * 64) {
    int4 raw[S];
#pragma unroll
    for (int q = 0; q < S; ++q) raw[q] = p[q * 64];                               // ds_read_b128, conflict-free
    double xv[S];
#pragma unroll
    for (int q = 0; q < S; ++q) xv[q] = *reinterpret_cast<const double *>(vec + (uint32_t)raw[q].z);   // gather
#pragma unroll
    for (int q = 0; q < S; ++q) out[q] = fma(__hiloint2double(raw[q].y, raw[q].x), xv[q], out[q]);
  }
  if (!LONG) return;
  for (int l = 0; l < ll.count; ++l) {
    const int owner = ll.owner[l], start = ll.start[l], len = ll.len[l];
    double part = 0.0;
    for (int t = lane; t < len; t += 64) {
      const int4 raw = *reinterpret_cast<const int4 *>(tail + start + t);
      part = fma(__hiloint2double(raw.y, raw.x), *reinterpret_cast<const double *>(vec + (uint32_t)raw.z), part);
    }
    part = wave_sum(part);
#pragma unroll
    for (int q = 0; q < S; ++q)
      if (owner == lane + 64 * q) out[q] += part;
  }
}

// Register-resident ELL (small LPs): the lane's W*S entries live in VGPRs for the whole kernel, so an SpMV is
// W*S independent LDS gathers issued back to back (one LDS latency instead of W dependent round trips) + W*S FMAs.
template <int S, unsigned PACK>
struct RegEll {
  static constexpr int w(int q) { return q < 8 ? (int)((PACK >> (4 * q)) & 15u) : 0; }   // width of slot q (<= 8 slots)
  static constexpr int base(int q) { int t = 0; for (int i = 0; i < q; ++i) t += w(i); return t; }
  static constexpr int total() { return base(S); }
  static constexpr int N = total() < 1 ? 1 : total();
  double v[N];
  uint32_t off[N];
  // `vec_lds` = LDS byte address of the exchange buffer this matrix gathers from: folded into the offsets once,
  // so a gather needs no address arithmetic in the iteration
  // The values are stored pre-multiplied by `scale` (the solve kernel folds its step size into the matrix).
  __device__ __forceinline__ void load(const Entry *__restrict__ g, int lane, uint32_t vec_lds, double scale) {
    // Two passes: ALL loads first, then the conversions.  (One pass - load, scale, fold the address, pin it with the asm
    // below - made every entry wait for its own load: total() serialised L2 round trips at every restart that changes the
    // weight, 16 on the 24-h shape = ~7800 cycles = 10 iterations, 28 on the 48-h one; tools/gpu_check_profile.py.)
    // The lane's byte offset is made opaque HERE: left to itself the compiler forms the total() entry addresses once per
    // kernel (they are loop-invariant), runs out of registers for them and reloads each from scratch before its load.  (The
    // offset, not the base address g + lane: that sum is loop-invariant too, was formed once per kernel, spilled, and came back
    // from scratch behind an s_waitcnt of its own in front of the loads of every restart.)
    uint32_t lane_off = (uint32_t)sizeof(Entry) * (uint32_t)lane;
#ifndef DSP_NO_OPAQUE_BASE
    asm volatile("" : "+v"(lane_off));
#endif
    const Entry *gl = reinterpret_cast<const Entry *>(reinterpret_cast<const char *>(g) + lane_off);
    typedef int v4i __attribute__((ext_vector_type(4)));                 // (a plain vector type: HIP's int4 class has no
    using gv4i = const __attribute__((address_space(1))) v4i;            //  assignment from an address-space-qualified source)
    gv4i *gp = (gv4i *)gl;
    v4i raw[N];
#pragma unroll
    for (int t = 0; t < total(); ++t) raw[t] = gp[t * 64];                                   // coalesced global loads
#pragma unroll
    for (int t = 0; t < total(); ++t) {
      v[t] = scale * __hiloint2double(raw[t].y, raw[t].x);
      off[t] = (uint32_t)raw[t].z + vec_lds;
      asm volatile("" : "+v"(off[t]));             // keep the folded address in a VGPR (no re-add per iteration)
    }
  }
  // The same re-read in two halves, for the restart block: fetch() issues the loads of the VALUES (the folded offsets do not
  // depend on the scale) as soon as a restart is decided, rescale() multiplies when the new weight is known - the L2 round trip
  // runs under the reduction and the weight update instead of after them.  v = scale * value, the multiplication of load().
  __device__ __forceinline__ void fetch(const Entry *__restrict__ g, int lane, double (&raw)[N]) const {
    uint32_t lane_off = (uint32_t)sizeof(Entry) * (uint32_t)lane;
    asm volatile("" : "+v"(lane_off));
    using gdbl = const __attribute__((address_space(1))) double;
    gdbl *gp = (gdbl *)(reinterpret_cast<const char *>(g) + lane_off);
#pragma unroll
    for (int t = 0; t < total(); ++t) raw[t] = gp[t * 64 * (int)(sizeof(Entry) / sizeof(double))];
  }
  __device__ __forceinline__ void rescale(double scale, const double (&raw)[N]) {
#pragma unroll
    for (int t = 0; t < total(); ++t) v[t] = scale * raw[t];
  }
  // out = init + (scaled matrix) * (vector in LDS); out and init may be the same array
  __device__ __forceinline__ void product(double (&out)[S], const double (&init)[S]) const {
    double xv[N];
#pragma unroll
    for (int t = 0; t < total(); ++t) xv[t] = lds_load_f64(off[t]);                          // ds_read_b64 gathers
#pragma unroll
    for (int q = 0; q < S; ++q) {
      double acc = init[q];
#pragma unroll
      for (int e = 0; e < w(q); ++e) acc = fma(v[base(q) + e], xv[base(q) + e], acc);
      out[q] = acc;
    }
  }
};

// long vectors only (their ELL entries are zero): cooperative wave reduction, tails in LDS
template <int S>
__device__ __forceinline__ void long_product(double (&out)[S], const char *vec, int lane, const LongList &ll,
                                             const Entry *__restrict__ tail, double scale) {
  for (int l = 0; l < ll.count; ++l) {
    const int owner = ll.owner[l], start = ll.start[l], len = ll.len[l];
    double part = 0.0;
    for (int t = lane; t < len; t += 64) {
      const int4 raw = *reinterpret_cast<const int4 *>(tail + start + t);
      part = fma(__hiloint2double(raw.y, raw.x), *reinterpret_cast<const double *>(vec + (uint32_t)raw.z), part);
    }
    part = wave_sum(part);
#pragma unroll
    for (int q = 0; q < S; ++q)
      if (owner == lane + 64 * q) out[q] = fma(scale, part, out[q]);
  }
}

// stage the shared matrix of one workgroup into LDS (16-byte copies)
__device__ __forceinline__ void stage_entries(Entry *dst, const Entry *__restrict__ src, int count) {
  int4 *d = reinterpret_cast<int4 *>(dst);
  const int4 *s = reinterpret_cast<const int4 *>(src);
  for (int t = threadIdx.x; t < count; t += blockDim.x) d[t] = s[t];
}

// ---- the fused, LDS-resident PDLP solve ---------------------------------------------------------------------
#ifndef DSP_MIN_WAVES_SMALL
#define DSP_MIN_WAVES_SMALL 2
#endif
// The metric kernel - the 24-h wind + battery LP, <4, 2, false, 0x1133, 0x44> - is compiled for THREE waves per SIMD (168 VGPRs): its
// plain-iteration loop stays free of scratch there and, since the check path lost its spills on the common paths, the third wave's
// latency hiding outweighs the spills of the rare blocks (profiles/HISTORY.md, "Three waves for the metric kernel, r81a").  That
// shape alone: it is the one this was measured on; at 168 VGPRs the nuclear 24-h kernel and the generic one gain scratch on paths
// that have none at two waves, and the padded <4, 2> shape holds 24 matrix entries per lane instead of 16.
constexpr bool three_waves_shape(int cpl, int rpl, unsigned wc, unsigned wr, bool qp) {
  return !qp && cpl == 4 && rpl == 2 && wc == 0x1133u && wr == 0x44u;
}
// Kernels whose plain iterations READ the Halpern anchor weight 1 / (k + 2) (SolveArgs::anchor_w) instead of computing it in every
// lane.  The metric kernel alone: at three waves per SIMD it is bound by VALU issue and the LDS pipe, not by a wave's own latency
// chain, and it is the one this was measured on; every other instantiation keeps its loop instruction for instruction.
constexpr bool anchor_table_shape(int cpl, int rpl, unsigned wc, unsigned wr, bool qp) {
  return three_waves_shape(cpl, rpl, wc, wr, qp);
}
// The one place that says which first passes are three-wave kernels as the HOST sees a launch (shape of the handle, long vectors, QP):
// their follow-up passes (certificates, re-certification) run the LIGHT instantiation of the generic kernel of the same <CPL, RPL>,
// compiled ahead of time for exactly these (light_fn).  Every other first pass holds 256 VGPRs like the generic kernel and keeps it.
constexpr bool three_waves_first_pass(int cpl, int rpl, unsigned wc, unsigned wr, bool lng, bool qp) {
  return !lng && three_waves_shape(cpl, rpl, wc, wr, qp);
}
#ifndef DSP_ONE_WAVE_FROM
#define DSP_ONE_WAVE_FROM 99      /* CPL + RPL from which the kernel is compiled for ONE wave per SIMD (512 registers: 256 V + 256 A) */
#endif
// WC / WR != 0: the ELL part of A^T / A is register-resident (RegEll); the template value packs the per-slot
// widths, 4 bits each, and ownership follows the sorted layout (P.mr_colat / P.mr_rowat);
// WC = WR = 0: generic path, matrix in LDS with run-time uniform widths, identity ownership.
// QP: rows with a compliance (dsp_batch::row_compliance) are soft - the dual step of every row is followed by the
// proximal shrink 1 / (1 + sig kappa_i) (= 1 for hard rows), the KKT test counts no violation for soft rows and adds the
// quadratic terms to both objectives.  A separate instantiation: the LP kernels pay nothing for it.
// A per-scenario value that only the rare blocks of the solve loop touch (KKT test, restart, ray jump, epilogue).  L = true
// (register-resident kernels): a lane-private copy in the wave's LDS region, read where it is used - kept in registers these
// values (2 RPL + 9 doubles per lane) are what the allocator spills first, and the rare blocks then reload them from scratch
// one memory round trip at a time.  L = false: a plain register (the LDS-matrix kernels run 8 waves per block).
#ifndef DSP_EARLY_MAT_UPTO
#define DSP_EARLY_MAT_UPTO 8
#endif
// Only the row bounds are per lane (slot k of the lane at + 512 k).  The nine values that are the same in every lane (norms,
// objective offset, weight guards, polish state, objective) have ONE 8-byte slot per wave at a wave-uniform address: every lane
// stores the same number, and what is read back is uniform to the compiler, so every test on it - and on the weight, the step
// sizes and the counters that depend on it - is a scalar branch (v_cmp + s_cbranch_vcc), not an EXEC-mask region.  Read from
// lane-private copies they made the whole check path, down to the hot loop's back edge, divergent in the compiler's eyes.
template <bool L>
struct Rare {
  double v;
  uint32_t addr;
  __device__ __forceinline__ double get() const { if constexpr (L) return lds_load_f64(addr); else return v; }
  __device__ __forceinline__ void set(double x) { if constexpr (L) lds_store_f64(addr, x); else v = x; }
};

// A wave-uniform flag of the solve loop.  PACK (the three-wave metric kernel): one bit of a word all of them share - kept as `bool`
// each is a 64-bit lane mask in two scalar registers through the whole solve, and the scalar file is what that kernel is short of.
// Every other kernel keeps the plain `bool` (wave_flag<false, BIT>), and with it its code, instruction for instruction.
template <unsigned BIT>
struct WaveFlag {
  unsigned &word;
  __device__ __forceinline__ operator bool() const { return (word >> BIT) & 1u; }
  __device__ __forceinline__ WaveFlag &operator=(bool v) { word = (word & ~(1u << BIT)) | ((unsigned)v << BIT); return *this; }
};
struct NoFlagWord {};
template <bool PACK, unsigned BIT> struct wave_flag {
  using type = bool;
  using word = NoFlagWord;
  static constexpr __device__ __forceinline__ bool make(NoFlagWord, bool v) { return v; }
};
template <unsigned BIT> struct wave_flag<true, BIT> {
  using type = WaveFlag<BIT>;
  using word = unsigned;
  static __device__ __forceinline__ WaveFlag<BIT> make(unsigned &w, bool v) { WaveFlag<BIT> f{w}; f = v; return f; }
};
#define DSP_WAVE_FLAG(NAME, BIT, INIT) typename wave_flag<ARGS_HERE, BIT>::type NAME = wave_flag<ARGS_HERE, BIT>::make(wave_flags, INIT)

// LIGHT (launch bounds only - the body is the same): the generic kernel as the FOLLOW-UP pass (certificates, re-certification) of a
// three-wave first pass, compiled for blocks of one wave at three waves per SIMD, so that a block fits the 168 VGPRs ONE leaving
// wave of the first pass sets free; at 256 VGPRs a wave needs two of a SIMD's three gone, a block of four that on one CU four times
// over, and the stream's next solve waits behind it.  It spills; it runs for suspects and flagged scenarios only.
template <int CPL, int RPL, bool LONG, unsigned WC, unsigned WR, bool QP = false, bool LIGHT = false>
__global__ void __launch_bounds__(LIGHT ? 64 : (CPL + RPL >= DSP_ONE_WAVE_FROM && WC != 0) ? 256 : 512, (LIGHT || three_waves_shape(CPL, RPL, WC, WR, QP)) ? 3 : (CPL + RPL <= 6) ? DSP_MIN_WAVES_SMALL : ((CPL + RPL >= DSP_ONE_WAVE_FROM && WC != 0) ? 1 : 2)) pdlp_solve_kernel(SolveArgs a) {
  constexpr bool MATREG = WC != 0;
  constexpr bool EARLY_MAT = MATREG && CPL + RPL <= DSP_EARLY_MAT_UPTO;   // restart block: matrix re-read issued ahead of the weight update
  constexpr bool RLDS = MATREG;                                        // rare per-scenario values in LDS (struct Rare)
  constexpr bool ANCHOR_TABLE = anchor_table_shape(CPL, RPL, WC, WR, QP);  // plain iterations: anchor weight from SolveArgs::anchor_w
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // after a simplex pass that certified every scenario there is nothing to do (one scalar load per wave)
  if (a.skip_solved == 1 && __builtin_amdgcn_readfirstlane(*a.unsolved) == 0) return;
  // certificate pass (below: CERT) after a register-resident kernel that left no suspect: nothing to do either
  if (a.skip_solved == 2 && __builtin_amdgcn_readfirstlane(*a.suspects) == 0) return;
  // re-certification pass (dsp_options::recertify_passes; generic kernels only) with no scenario left flagged DSP_FLAG_OBJ_WAIVED: nothing to do
  if constexpr (!MATREG) if (a.skip_solved == 3 && __builtin_amdgcn_readfirstlane(a.suspects[2]) == 0) return;
  // Infeasibility / unboundedness certificates (dsp_options::eps_infeasible).  The generic kernels evaluate them themselves, at
  // restarts.  The register-resident kernels do NOT carry that code: on the 48-h shape - 246 of 256 VGPRs are live state - the two
  // extra products in a rare block made the allocator spill on the common paths (-10 % on the whole batch, -2 % on the 24-h
  // metric kernel, wherever the block was put: profiles/r50p_*, tools/kernel_resources.sh).  They only WATCH the relative gap (one
  // comparison per KKT test) and hand a scenario whose objectives keep drifting apart over three tests to a second launch of the
  // generic kernel (skip_solved = 2), which continues from its iterate.  Feasible batches: that launch returns at the line above.
  constexpr bool CERT = !MATREG;
  const DeviceProblem &P = a.P;
  const KernelBatch &b = a.b;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (wave-uniform, and known to be)

  // ---- carve LDS: shared matrix region, then one exchange buffer pair per wave ----------------------------
  Entry *ellc = reinterpret_cast<Entry *>(smem);                       // A^T (columns)  [Wc*CPL*64]
  Entry *ellr = ellc + (MATREG ? 0 : P.ellc_entries);                  // A   (rows)     [Wr*RPL*64]
  Entry *tailc = ellr + (MATREG ? 0 : P.ellr_entries);
  const int n_tailc = MATREG ? P.mr_tailc_entries : P.tailc_entries;
  const int n_tailr = MATREG ? P.mr_tailr_entries : P.tailr_entries;
  Entry *tailr = tailc + n_tailc;
  char *wave_buf = reinterpret_cast<char *>(tailr + n_tailr);          // [waves][(n_pad + m_pad) * 8]
  if (!MATREG) {
    stage_entries(ellc, P.ellc, P.ellc_entries);
    stage_entries(ellr, P.ellr, P.ellr_entries);
  }
  stage_entries(tailc, MATREG ? P.mr_tailc : P.tailc, n_tailc);
  stage_entries(tailr, MATREG ? P.mr_tailr : P.tailr, n_tailr);
  const LongList &long_c = MATREG ? P.mr_long_c : P.long_c;
  const LongList &long_r = MATREG ? P.mr_long_r : P.long_r;
  // Scale factors of the owned columns / rows, [CPL + RPL][64] doubles behind the waves' exchange buffers (every wave writes
  // the same values): the KKT test measures its residuals in the unscaled space.  Read from global memory where they are
  // used (`j >= 0 ? P.col_scale[j] : 1`: slot -> index -> factor), the compiler gave every slot its own block behind its own
  // s_waitcnt - 2 (CPL + RPL) serialised L2 round trips per test, ~7 us on the 24-h shape = 16 iterations - and kept doing so
  // when the loads were written branch-free ahead of the products (register pressure: one address / result pair at a time).
  const uint32_t scl_lds = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char *)(wave_buf + (size_t)(blockDim.x >> 6) * ((size_t)(P.n_pad + P.m_pad) * 8 + (MATREG ? rare_lds_bytes(RPL) : 0))) + 8u * (uint32_t)lane;
  DSP_TRACE("[trace] staged: Wc=%d Wr=%d B=%d maxit=%d\n", P.Wc, P.Wr, b.B, a.opt.max_iter);

  const size_t wave_stride = (size_t)(P.n_pad + P.m_pad) * 8 + (RLDS ? rare_lds_bytes(RPL) : 0);
  char *xb = wave_buf + (size_t)wave * wave_stride;                    // gathered by row products
  char *yb = xb + (size_t)P.n_pad * 8;                                 // gathered by column products
  // LDS byte addresses of this lane's own elements in the exchange buffers (permuted slots: dsp_prepare.hpp, optimise_slots)
  using lds_cptr = const __attribute__((address_space(3))) char *;
  const uint32_t xb_lds = (uint32_t)(uintptr_t)(lds_cptr)xb, yb_lds = (uint32_t)(uintptr_t)(lds_cptr)yb;
  const uint32_t rare_lds = yb_lds + 8u * (uint32_t)P.m_pad + 8u * (uint32_t)lane;   // per-lane slot k of struct Rare at + 512 k
  const uint32_t rare_uni = yb_lds + 8u * (uint32_t)P.m_pad + 1024u * RPL;           // wave-uniform slot k at + 8 k
  static_assert(!RLDS || rare_lds_bytes(RPL) == 1024 * RPL + 8 * 9, "host LDS sizing (dsp_capi.hip) and the layout of struct Rare disagree");
  // SHARED (shapes with more than 8 owned elements per lane): the host built the same slot map for every 64-position block,
  // so ONE address register per buffer + the compile-time offsets 512 q serve all owned elements (the stores pair up into
  // ds_write2_b64); with one address VGPR per element the 48-h kernel reloaded three of them from scratch EVERY iteration
  // (768 B per scenario-iteration: 12 GB of fetches per 4096-scenario launch, profiles/r03c48_pmc_summary.csv).
  constexpr bool SHARED = MATREG && shared_slot_maps(CPL, RPL);
  uint32_t xw[CPL], yw[RPL];
  if constexpr (SHARED) {
    xw[0] = xb_lds + 8u * (uint32_t)P.mr_slot_x[lane];
    yw[0] = yb_lds + 8u * (uint32_t)P.mr_slot_y[lane];
    asm volatile("" : "+v"(xw[0]));
    asm volatile("" : "+v"(yw[0]));
#pragma unroll
    for (int q = 1; q < CPL; ++q) xw[q] = xw[0] + 512u * q;
#pragma unroll
    for (int q = 1; q < RPL; ++q) yw[q] = yw[0] + 512u * q;
  } else {
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      xw[q] = xb_lds + 8u * (uint32_t)(MATREG ? P.mr_slot_x[lane + 64 * q] : lane + 64 * q);
      asm volatile("" : "+v"(xw[q]));                // opaque: keeps the address in a VGPR instead of re-adding it per store
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
      yw[q] = yb_lds + 8u * (uint32_t)(MATREG ? P.mr_slot_y[lane + 64 * q] : lane + 64 * q);
      asm volatile("" : "+v"(yw[q]));
    }
  }
  RegEll<CPL, WC> mreg_c;                                                // tau A^T, gathers y from yb   } loaded per
  RegEll<RPL, WR> mreg_r;                                                // -sig A, gathers x from xb    } scenario / weight

  const int n = P.n, m = P.m;
  // column / row owned by slot q of this lane (-1 = padding): sorted layout for the register-resident kernel
  auto col_id = [&](int q) __attribute__((always_inline)) {
    if constexpr (MATREG) return P.mr_colat[lane + 64 * q];
    else { const int j = lane + 64 * q; return j < n ? j : -1; }
  };
  auto row_id = [&](int q) __attribute__((always_inline)) {
    if constexpr (MATREG) return P.mr_rowat[lane + 64 * q];
    else { const int i = lane + 64 * q; return i < m ? i : -1; }
  };
  static_assert(scale_lds_bytes(CPL, RPL) == (CPL + RPL) * 512, "host LDS sizing (dsp_capi.hip) and the table layout below disagree");
#pragma unroll
  for (int q = 0; q < CPL; ++q) { const int j = col_id(q); lds_store_f64(scl_lds + 512u * q, j >= 0 ? P.col_scale[j] : 1.0); }
#pragma unroll
  for (int q = 0; q < RPL; ++q) { const int i = row_id(q); lds_store_f64(scl_lds + 512u * (CPL + q), i >= 0 ? P.row_scale[i] : 1.0); }
  __syncthreads();
  const double eta = a.eta;
  const double eps = a.opt.eps_rel;
  const double eps_obj = a.opt.eps_obj;
  // check_every = 0: automatic - 16, or 32 for shapes with more than 8 owned elements per lane (the 48-h wind+battery LP:
  // 246 of 256 VGPRs are live state and the rare blocks of its check - KKT test, restart, ray jump - still spill; a check
  // costs ~10 iterations there against ~7 on the 24-h shape, and every second check saved is worth more than the ~7 %
  // extra iterations of the coarser restart cadence: profiles/r03d_check_every_48h.log, re-measured r04z_rare2.log)
  const int check_every = a.opt.check_every > 0 ? a.opt.check_every : (CPL + RPL > 8 ? 32 : 16);
  const int kkt_every = a.opt.kkt_every > 0 ? a.opt.kkt_every : 1;
  // the restart / steady tests on SQUARED residuals: r <= beta r0  <=>  r^2 <= beta^2 r0^2,
  // |r - rprev| <= s r  <=>  (1 - s)^2 r^2 <= rprev^2 <= (1 + s)^2 r^2
  // These factors (and 1 / eta) are formed WHERE THEY ARE USED, from the kernel arguments (scalar registers): computed once up
  // here they are wave-uniform doubles that sit in VGPRs through the whole solve, the register file is full, and they are what the
  // allocator spills - four scratch reloads, each behind its own s_waitcnt, on the path of every check.  `opt_here` keeps the
  // compiler from hoisting them back out of the loop.
  auto opt_here = [](double v) __attribute__((always_inline)) { asm volatile("" : "+s"(v)); return v; };
  // ARGS_HERE (the three-wave metric kernel): the options of the restart, steady and ray-jump tests are LOADED where they are used,
  // from the kernel-argument segment through the scalar data cache.  Held in scalar registers from the kernel's entry they - and the
  // comparisons on them the compiler forms up there, 64-bit lane masks each - are spilled to VGPR lanes, and the allocator brings a
  // spilled argument back eight registers at a time, the s_load_dwordx8 it arrived in: 57 v_readlane_b32, VALU-issued in all 64
  // lanes, on the path of a check on which nothing fires.  `args_here` makes the segment's address opaque, so that nothing read
  // through it is hoisted back; the loads return where no LDS gather is in flight.
  constexpr bool ARGS_HERE = three_waves_shape(CPL, RPL, WC, WR, QP);
  using args_ptr = const __attribute__((address_space(4))) char *;
  auto args_here = []() __attribute__((always_inline)) {
    args_ptr p = (args_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
  };
#define DSP_ARG(p, member) (*(const __attribute__((address_space(4))) decltype(SolveArgs::member) *)((p) + __builtin_offsetof(SolveArgs, member)))
#define DSP_OPT(p, field) (*(const __attribute__((address_space(4))) decltype(dsp_options::field) *)((p) + __builtin_offsetof(SolveArgs, opt) + __builtin_offsetof(dsp_options, field)))
#define DSP_OPT_HERE(field) (ARGS_HERE ? DSP_OPT(ka, field) : a.opt.field)
#define DSP_OPT_F64(field) (ARGS_HERE ? DSP_OPT(ka, field) : opt_here(a.opt.field))
#define DSP_OPT_LOADED(loaded, argument) (ARGS_HERE ? (loaded) : (argument))      /* a value the ARGS_HERE kernel loaded in a batch */
  // The step sizes are folded into the products: out = init + tau A^T (vector in yb) and out = init - sig A (vector in
  // xb).  Register-resident matrices hold tau A^T / -sig A themselves, so a PDHG half-step is the FMA chain alone;
  // the LDS matrix is shared by the block's waves (each with its own weight) and is scaled on the way out.
  auto col_step = [&](double (&out)[CPL], const double (&init)[CPL], double tau_) __attribute__((always_inline)) {
    if constexpr (MATREG) {
      mreg_c.product(out, init);
      if (LONG) long_product<CPL>(out, yb, lane, long_c, tailc, tau_);
    } else {
      double pr[CPL];
      ell_product<CPL, LONG>(pr, ellc, P.Wc, yb, lane, P.long_c, tailc);
#pragma unroll
      for (int q = 0; q < CPL; ++q) out[q] = fma(tau_, pr[q], init[q]);
    }
  };
  auto row_step = [&](double (&out)[RPL], const double (&init)[RPL], double nsig_) __attribute__((always_inline)) {
    if constexpr (MATREG) {
      mreg_r.product(out, init);
      if (LONG) long_product<RPL>(out, xb, lane, long_r, tailr, nsig_);
    } else {
      double pr[RPL];
      ell_product<RPL, LONG>(pr, ellr, P.Wr, xb, lane, P.long_r, tailr);
#pragma unroll
      for (int q = 0; q < RPL; ++q) out[q] = fma(nsig_, pr[q], init[q]);
    }
  };
  const double zero_c[CPL] = {}, zero_r[RPL] = {};

#ifdef DSP_PROF     /* development: where a wave's cycles go - hot loop / check base / KKT test / restart / ray jump (tools/gpu_check_profile.py) */
  long long prof_c[6] = {0, 0, 0, 0, 0, 0}, prof_n[6] = {0, 0, 0, 0, 0, 0}, prof_t = 0;
#define DSP_PROF_MARK() prof_t = clock64();
#define DSP_PROF_ADD(i) { const long long t_ = clock64(); prof_c[i] += t_ - prof_t; ++prof_n[i]; prof_t = t_; }
#else
#define DSP_PROF_MARK()
#define DSP_PROF_ADD(i)
#endif
#ifdef DSP_CLOCKS   /* development: shader clock vs constant 100 MHz clock, cycles per wave-iteration */
  const long long clk0 = clock64(), wall0 = wall_clock64();
  long long iters_done = 0;
#endif
  for (;;) {
    // ---- pull the next scenario off the work queue ---------------------------------------------------------
    // EVERY lane takes part in the atomic (lane 0 adds 1, the others 0; the compiler's atomic optimiser turns that into
    // one global atomic per wave) and the ticket is read from lane 0 explicitly.  Round 1 wrote
    //     if (lane == 0) s = atomicAdd(queue, 1);  s = readfirstlane(s);
    // and needed an s_waitcnt 0 after the result stores at the bottom of the loop "against a hang".  Root cause (round 2,
    // profiles/r02d_drain_modes.log (seven builds bisecting the drains): a compiler-only barrier `asm volatile("" ::: "memory")` in place of that s_waitcnt cures it
    // just as well, so no memory ordering is involved): the loop body ends with `if (lane == 0) { stores }` and began with
    // `if (lane == 0) { atomic }`; with nothing side-effecting in between, the compiler threads the divergent
    // `lane == 0` branch across the back-edge, the wave re-enters the pull with a partial EXEC mask, v_readfirstlane
    // returns the value of a lane that did not run the atomic (s = 0), and every wave re-solves scenario 0 for ever -
    // "hung at the end of the first scenario of every wave".  A pull without a divergent branch and without
    // readfirstlane has nothing to thread and does not depend on EXEC.
#ifdef DSP_LEGACY_PULL
    int s = 0;
    if (lane == 0) s = (int)((unsigned)atomicAdd(a.queue, 1) - a.queue_base);   
    s = __builtin_amdgcn_readfirstlane(s);
#else
    __builtin_amdgcn_wave_barrier();
    const int ticket = (int)((unsigned)atomicAdd(a.queue, lane == 0 ? 1 : 0) - a.queue_base);
    const int s = __builtin_amdgcn_readlane(ticket, 0);
#endif
    DSP_TRACE("[trace] scenario %d\n", s);
    if ((unsigned)s >= (unsigned)b.B) break;
    if (a.skip_solved == 1 && __builtin_amdgcn_readfirstlane(b.status[s]) != DSP_STATUS_UNSOLVED) continue;
    if (a.skip_solved == 2 && __builtin_amdgcn_readfirstlane(b.status[s]) != DSP_STATUS_SUSPECT) continue;
    // re-certification pass: only scenarios the earlier passes accepted WITHOUT a certified objective accuracy, from a cold start under
    // this launch's options (another restart cadence / weight controller: dsp_capi.hip, recertify_passes)
    if constexpr (!MATREG) if (a.skip_solved == 3 && !(__builtin_amdgcn_readfirstlane(b.status[s]) == DSP_STATUS_OPTIMAL && (__builtin_amdgcn_readfirstlane(b.flags[s]) & DSP_FLAG_OBJ_WAIVED))) continue;
    // (certificate pass: the iterations the first pass spent on the scenario count; the limit covers both passes.  Re-certification:
    //  they count too, the limit is this pass's own)
    const int it_base = ((MATREG ? a.skip_solved == 2 : a.skip_solved >= 2) && b.iters) ? __builtin_amdgcn_readfirstlane(b.iters[s]) : 0;
    const int max_it = (!MATREG && a.skip_solved == 3) ? a.opt.max_iter : max(a.opt.max_iter - it_base, 1);

    // ---- load + scale this scenario's vectors (coalesced: lane-consecutive addresses) -----------------------
    double x[CPL], x0[CPL], c[CPL], lb[CPL], ub[CPL];
    double y[RPL], y0[RPL];
    Rare<RLDS> rlo[RPL], rhi[RPL], qn, cn, c0, w_lo, w_hi, w_init, pol_best, pol_po, pobj;
    {
      int k_ = 0;
#pragma unroll
      for (int q = 0; q < RPL; ++q) rlo[q].addr = rare_lds + 512u * (k_++);
#pragma unroll
      for (int q = 0; q < RPL; ++q) rhi[q].addr = rare_lds + 512u * (k_++);
      k_ = 0;
      qn.addr = rare_uni + 8u * (k_++); cn.addr = rare_uni + 8u * (k_++); c0.addr = rare_uni + 8u * (k_++);
      w_lo.addr = rare_uni + 8u * (k_++); w_hi.addr = rare_uni + 8u * (k_++); w_init.addr = rare_uni + 8u * (k_++);
      pol_best.addr = rare_uni + 8u * (k_++); pol_po.addr = rare_uni + 8u * (k_++); pobj.addr = rare_uni + 8u * (k_++);
    }
    double kap[QP ? RPL : 1], srow[QP ? RPL : 1];        // QP: scaled compliance kappa d_r^2 and 1 / (1 + sig kappa)
    double nrm[4] = {0.0, 0.0, 0.0, 0.0};                // |q|^2 unscaled, |c|^2 unscaled, |q|^2 scaled, |c|^2 scaled
    double cmax = 0.0, qmax = 0.0;                       // largest scaled |c_j| / finite scaled |row bound|
    double bs2 = 0.0;                                    // sum of squared finite scaled column bounds
    double bad = 0.0;                                    // > 0: crossed bounds (lb > ub or row_lb > row_ub) or NaN input
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      const int j = col_id(q);
      const bool ok = j >= 0;
      const double d = ok ? P.col_scale[j] : 1.0;
      const double cu = ok ? b.c[(size_t)s * b.c_stride + j] : 0.0;
      const double lu = ok ? (b.var_lb ? b.var_lb[(size_t)s * b.var_lb_stride + j] : -INFINITY) : 0.0;
      const double uu = ok ? (b.var_ub ? b.var_ub[(size_t)s * b.var_ub_stride + j] : INFINITY) : 0.0;
      c[q] = cu * d;
      lb[q] = lu / d;
      ub[q] = uu / d;
      nrm[1] += cu * cu;
      if (!(lu <= uu) || !(cu == cu)) bad = 1.0;
      nrm[3] += c[q] * c[q];
      cmax = fmax(cmax, fabs(c[q]));
      { const double lfs = finite_or_zero(lb[q]), ufs = finite_or_zero(ub[q]); bs2 += lfs * lfs + ufs * ufs; }
      const double lf = finite_or_zero(lu), uf = finite_or_zero(uu);
      nrm[0] += lf * lf + uf * uf;
      const double xs = (b.x0 && ok) ? b.x0[(size_t)s * n + j] / d : 0.0;
      x[q] = clampd(xs, lb[q], ub[q]);
      x0[q] = x[q];
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
      const int i = row_id(q);
      const bool ok = i >= 0;
      const double d = ok ? P.row_scale[i] : 1.0;
      const double lo = (ok && b.row_lb) ? b.row_lb[(size_t)s * b.row_lb_stride + i] : -INFINITY;
      const double hi = (ok && b.row_ub) ? b.row_ub[(size_t)s * b.row_ub_stride + i] : INFINITY;
      const double rlo_q = lo * d, rhi_q = hi * d;
      rlo[q].set(rlo_q);
      rhi[q].set(rhi_q);
      if (!(lo <= hi)) bad = 1.0;
      if constexpr (QP) {
        const double kp_ = ok ? a.b.row_compliance[(size_t)s * a.b.row_compliance_stride + i] : 0.0;
        kap[q] = kp_ * d * d;
        // a soft row is the term (a.x - b)^2 / (2 kappa): it needs ONE finite target b = row_lb = row_ub
        if (!(kp_ >= 0.0) || (kp_ > 0.0 && !(lo == hi && is_finite(lo)))) bad = 1.0;
      }
      const double big = fmax(fabs(finite_or_zero(lo)), fabs(finite_or_zero(hi)));
      nrm[0] += big * big;
      const double bigs = fmax(fabs(finite_or_zero(rlo_q)), fabs(finite_or_zero(rhi_q)));
      nrm[2] += bigs * bigs;
      qmax = fmax(qmax, bigs);
      double ys = (b.y0 && ok) ? b.y0[(size_t)s * m + i] / d : 0.0;
      // keep the warm start dual-feasible in sign
      if (!is_finite(rlo_q)) ys = fmin(ys, 0.0);
      if (!is_finite(rhi_q)) ys = fmax(ys, 0.0);
      y[q] = ys;
      y0[q] = ys;
    }
    wave_sums<4>(nrm);
    if (wave_max(bad) > 0.0) {
      // trivially infeasible / invalid scenario: report it and take the next one (nothing is iterated)
#pragma unroll
      for (int q = 0; q < CPL; ++q) { const int j = col_id(q); if (j >= 0) b.x[(size_t)s * n + j] = NAN; }
#pragma unroll
      for (int q = 0; q < RPL; ++q) { const int i = row_id(q); if (i >= 0) b.y[(size_t)s * m + i] = NAN; }
      if (lane == 0) {
        b.obj[s] = NAN;
        b.status[s] = (nrm[0] == nrm[0] && nrm[1] == nrm[1]) ? DSP_STATUS_PRIMAL_INFEASIBLE : DSP_STATUS_NUMERICAL;
        if (b.iters) b.iters[s] = 0;
        if (b.jumps) b.jumps[s] = 0;
        if (b.flags) b.flags[s] = 0;
      }
      continue;
    }
    qn.set(sqrt(nrm[0]));
    cn.set(sqrt(nrm[1]));
    const double qs = sqrt(nrm[2]), cs = sqrt(nrm[3]);
    c0.set(b.obj_offset ? b.obj_offset[(size_t)s * b.obj_offset_stride] : 0.0);
    double w = (cs > 1e-10 && qs > 1e-10) ? cs / qs : 1.0;       // primal weight
    // Rounding guard: the primal step tau = eta / w amplifies the rounding error of (c - A^T y), about 1.1e-16 |c|_max,
    // into x; once that noise reaches the primal tolerance the iteration stalls (seen when the dual has converged to
    // machine precision and the movement-ratio controller keeps shrinking w).  Keep tau u |c|_max <= eps (1 + |q|) /
    // guard (|q| = all finite row and column bounds), and symmetrically sigma u |q|_max <= eps (1 + |c|) / guard.
    cmax = wave_max(cmax);
    qmax = wave_max(qmax);
    const double qall = sqrt(nrm[2] + wave_sum(bs2));       // row AND column bounds (the scale of the primal test)
    // (not const: the polish phase tightens the guard on the noisy side, see the KKT block)
    w_lo.set(a.opt.weight_guard > 0.0 ? a.opt.weight_guard * eta * 1.1e-16 * cmax / (eps * (1.0 + qall)) : 0.0);
    w_hi.set((a.opt.weight_guard > 0.0 && qmax > 0.0)
                 ? eps * (1.0 + cs) / (a.opt.weight_guard * eta * 1.1e-16 * qmax) : INFINITY);
    w_init.set(w);                   // the AUTOMATIC weight: what a stalled weight is pulled back to, and where a given-up warm start starts again
    if (b.primal_weight) {
      const double wi = b.primal_weight[s];
      if (wi > 0.0 && is_finite(wi)) w = wi;
    }
    // warm start on patience (dsp_options::warm_patience): started from the caller's point, not terminated after that many iterations ->
    // once more from the cold point at the next check (the restart block)
    typename wave_flag<ARGS_HERE, 0>::word wave_flags{};      // (ARGS_HERE: the five flags below, one bit each)
    DSP_WAVE_FLAG(warm, 0, a.opt.warm_patience > 0 && a.skip_solved == 0 && (b.x0 != nullptr || b.y0 != nullptr));      // (first pass only: the later passes' x0 is the pass before)

    DSP_TRACE("[trace] loaded w=%g\n", w);
    int k = 0;                       // iterations since the last restart
    int it = 0;
    int it0 = 0;                     // iteration the current start was made at (> 0: a warm start given up, dsp_options::warm_patience)
    int njump = 0;
    int ncheck = 0, last_kkt = 0;
    double gate2 = 0.0;              // the next gated KKT test runs once r^2 <= gate2
    int jump_not_before = 0;         // no ray-jump test while k (iterations since the anchor reset) is below this
    int stalls = 0;                  // restarts forced after >= stall_rescue iterations without decay
    DSP_WAVE_FLAG(waive_obj, 1, false);    // stalled twice: terminate on the eps_rel tests alone
    DSP_WAVE_FLAG(lastjump, 2, false);    // the last restart of the anchor was a ray jump
    DSP_WAVE_FLAG(suspect, 3, false);    // the last KKT test found the objectives drifting apart: KKT tests at every 4th check from then on
    int nsus = 0;                    // consecutive KKT tests that did (register-resident kernels: three of them end the first pass)
    pol_best.set(INFINITY);          // polish phase (eps_rel tests hold, eps_obj tests missing): best worst-ratio seen,
    int pol_it = 0, nboost = 0;      //   the iteration it was seen at, guard tightenings so far
    DSP_WAVE_FLAG(pol_tried, 4, false);    //   the guard test of this stagnation period has been made
    pol_po.set(0.0);                 //   primal objective when the best ratio was seen
#ifdef DSP_KKT_TRACE
    int ntrace = 0;
#endif
    double r0 = INFINITY, rprev = INFINITY;      // SQUARED residuals (no square root on the check path)
    int status = DSP_STATUS_ITERATION_LIMIT;
    double xp[CPL], yp[RPL];
    pobj.set(0.0);
#pragma unroll
    for (int q = 0; q < CPL; ++q) xp[q] = x[q];
#pragma unroll
    for (int q = 0; q < RPL; ++q) yp[q] = y[q];

// one PDHG application T(x, y) -> (xp, yp).  The unprojected points gx = x - tau (c - A^T y), gy = y - sig A (2 x+ - x) are
// temporaries: the ray jump, the only other user, recomputes them in the ~1 attempt in 10 that reaches its ratio test
// (kept live across the check they pinned 2 (CPL + RPL) VGPRs through the KKT block: scratch traffic on the 48-h shape)
#define DSP_PDHG_STEP()                                                                                     \
  {                                                                                                         \
    _Pragma("unroll") for (int q = 0; q < RPL; ++q) lds_store_f64(yw[q], y[q]);                             \
    wave_lds_fence();                                                                                       \
    double gx[CPL], gy[RPL];                                                                                \
    _Pragma("unroll") for (int q = 0; q < CPL; ++q) gx[q] = fma(-tau, c[q], x[q]);                          \
    col_step(gx, gx, tau);                                                                                  \
    _Pragma("unroll") for (int q = 0; q < CPL; ++q) {                                                       \
      xp[q] = clampd(gx[q], lb[q], ub[q]);                                                                  \
      lds_store_f64(xw[q], 2.0 * xp[q] - x[q]);                                                             \
    }                                                                                                       \
    wave_lds_fence();                                                                                       \
    row_step(gy, y, -sig);                                                                                  \
    _Pragma("unroll") for (int q = 0; q < RPL; ++q) {                                                       \
      yp[q] = gy[q] - clampd_bare(gy[q], ylo[q], yhi[q]);                                                   \
      if constexpr (QP) yp[q] *= srow[q];                                                                   \
    }                                                                                                       \
  }
// reflected Halpern step toward the anchor (x0, y0)
/* anchor weight 1/(k+2): the bare v_rcp_f64 (no Newton step); Halpern needs the weight, not its last bits */
#define DSP_ANCHOR_WEIGHT() __builtin_amdgcn_rcp((double)(k + 2))
#define DSP_HALPERN_STEP(WEIGHT)                                                                            \
  {                                                                                                         \
    const double oml = WEIGHT;                                                                              \
    _Pragma("unroll") for (int q = 0; q < CPL; ++q) {                                                       \
      const double t = 2.0 * xp[q] - x[q];                                                                  \
      x[q] = fma(oml, x0[q] - t, t);                                                                        \
    }                                                                                                       \
    _Pragma("unroll") for (int q = 0; q < RPL; ++q) {                                                       \
      const double t = 2.0 * yp[q] - y[q];                                                                  \
      y[q] = fma(oml, y0[q] - t, t);                                                                        \
    }                                                                                                       \
  }
    // step sizes, the clamp window of the dual update (y+ = v - clamp(v, -sig rhi, -sig rlo), v = y - sig A(2x+ - x))
    // and the step-scaled register matrices: functions of the primal weight, refreshed only where it changes (one FP64
    // division; the matrices are re-read from L2, 16 bytes per entry and lane, so they stay exact)
    double tau, sig, iw, ylo[RPL], yhi[RPL];
#define DSP_SET_STEPS() { DSP_SET_SCALARS() DSP_SET_MATRICES() }
#define DSP_SET_MATRICES()                                                                                  \
  {                                                                                                         \
    if constexpr (MATREG) {                                                                                 \
      mreg_c.load(P.mr_ellc, lane, yb_lds, tau);                                                            \
      mreg_r.load(P.mr_ellr, lane, xb_lds, -sig);                                                           \
    }                                                                                                       \
  }
#define DSP_SET_SCALARS()                                                                                   \
  {                                                                                                         \
    iw = 1.0 / w;                                                                                           \
    tau = eta * iw;                                                                                         \
    sig = eta * w;                                                                                          \
    _Pragma("unroll") for (int q = 0; q < RPL; ++q) { ylo[q] = -(sig * rhi[q].get()); yhi[q] = -(sig * rlo[q].get()); } \
    if constexpr (QP) { _Pragma("unroll") for (int q = 0; q < RPL; ++q) srow[q] = 1.0 / fma(sig, kap[q], 1.0); } \
  }
    DSP_SET_STEPS()
    DSP_TRACE("[trace] enter loop\n");
    for (it = 0;;) {
      // ---- plain iterations up to the next check: two SpMVs + elementwise work, no reduction, no branch --------
      const int plain = min(check_every - 1, max_it - it);
      DSP_PROF_MARK()
      // (today's loop: the anchor weight computed in every lane)
#define DSP_PLAIN_ITERATIONS()                                                                              \
  for (int u = 0; u < plain; ++u) {                                                                         \
    DSP_PDHG_STEP()                                                                                         \
    ++k;                                                                                                    \
    DSP_HALPERN_STEP(DSP_ANCHOR_WEIGHT())                                                                   \
  }
      if constexpr (ANCHOR_TABLE) {
        // (a flag, not if / else: written as else-branch the fallback loop gives the whole kernel another register allocation -
        //  392 B of scratch instead of 384 - which is not the one that was measured; profiles/r83a_kernel_resources.txt)
        bool computed = true;
        // Every weight of the segment lies in the table (a wave-uniform choice): the plain iterations read it through the scalar data
        // cache at a uniform address - no v_cvt_f64_i32 + v_rcp_f64, a quarter-rate VALU slot in all 64 lanes for one number per wave.
        // The weights are the bits DSP_ANCHOR_WEIGHT() gives (anchor_weight_kernel, dsp_capi.hip).
        // Scalar loads return through the counter of the LDS gathers, out of order: where the compiler knows one to be in flight it
        // turns every counted wait of a product's FMA chain into a wait for ALL its gathers, and left to itself it issues the load
        // right in front of its use.  So the load of the NEXT iteration's weight is written as the instruction, tied behind the
        // second product's last result and in front of every use of this iteration's weight: it runs under the Halpern step and is
        // waited for at the bottom of the body, where no gather is in flight (anchor_w has kAnchorWeights + 1 entries: the last
        // iteration loads one it does not use).
        if (k + plain <= kAnchorWeights) {
          computed = false;
          using cdbl = const __attribute__((address_space(4))) double;
          cdbl *aw = (cdbl *)a.anchor_w + k;
          double wk = aw[0];
          asm volatile("" : "+s"(wk));                 // (waited for HERE: in flight at the loop's entry it costs the first product its counted waits)
          for (int u = 0; u < plain; ++u) {
            DSP_PDHG_STEP()
            double wn;
            asm volatile("s_load_dwordx2 %0, %2, 0x0" : "=&s"(wn), "+s"(wk) : "s"(aw + u + 1), "v"(yp[RPL - 1]));
            DSP_HALPERN_STEP(wk)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(wn), "+v"(y[RPL - 1]));
            wk = wn;
          }
          k += plain;
        }
        if (computed) DSP_PLAIN_ITERATIONS()
      } else DSP_PLAIN_ITERATIONS()
#undef DSP_PLAIN_ITERATIONS
      DSP_PROF_ADD(0)
      it += plain;
      DSP_TRACE("[trace] it=%d k=%d\n", it, k);
      if (it >= max_it) break;
      // ---- check iteration ----------------------------------------------------------------------------------
      DSP_PDHG_STEP()
      ++k;
      bool moved = false;            // restarted or jumped: the Halpern step is skipped
      bool boost_now = false;        // polish phase: the weight guard was tightened at this check -> restart from here
      {
        // ---- every check: fixed-point residual in the PDHG metric (one SpMV, ONE reduction) ---------------------
        // |dz|^2_M = w |dx|^2 - 2 eta dy.A dx + |dy|^2 / w with -2 eta dy.A dx = 2 dy.(-sig A dx) / w  (sig = eta w):
        // a linear combination with wave-uniform weights, so the lanes combine their three partial sums first.
        // r is kept squared: every test below compares ratios.
        double px = 0.0, py = 0.0;
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
          const double dx = xp[q] - x[q];
          px = fma(dx, dx, px);
          lds_store_f64(xw[q], dx);
        }
        wave_lds_fence();
        double adx[RPL];
        row_step(adx, zero_r, -sig);                   // -sig A (x+ - x)
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
          const double dy = yp[q] - y[q];
          py = fma(dy, fma(2.0, adx[q], dy), py);
        }
        // (ARGS_HERE: the two options of the gate, requested ahead of the reduction and waited for behind it)
        args_ptr ka = nullptr;
        double kkt_gate = 0.0;
        int kkt_every_ = 0;
        if constexpr (ARGS_HERE) { ka = args_here(); kkt_gate = DSP_OPT(ka, kkt_gate); kkt_every_ = DSP_OPT(ka, kkt_every); }
        const double r = fmax(wave_sum(fma(w, px, iw * py)), 0.0);
        if constexpr (ARGS_HERE) { asm volatile("" : "+s"(kkt_gate), "+s"(kkt_every_)); kkt_every_ = kkt_every_ > 0 ? kkt_every_ : 1; }
        if (!(r == r)) { status = DSP_STATUS_NUMERICAL; break; }
        // ---- KKT test at (x+, y+) in the ORIGINAL (unscaled) space: 7 reductions + two SpMVs, so it is scheduled from
        // r, which the restart test has anyway (see dsp_options::kkt_gate); kkt_gate = 0: every kkt_every-th check
        ++ncheck;
        const bool kkt_now = (DSP_OPT_LOADED(kkt_gate, a.opt.kkt_gate) > 0.0
                                  ? (ncheck - last_kkt >= (last_kkt ? DSP_OPT_LOADED(kkt_every_, kkt_every) : min(4, DSP_OPT_LOADED(kkt_every_, kkt_every))) || r <= gate2)
                                  : (ncheck % DSP_OPT_LOADED(kkt_every_, kkt_every)) == 0) || (suspect && (ncheck & 3) == 0);
        DSP_PROF_ADD(1)
        if (kkt_now) {
#pragma unroll
          for (int q = 0; q < RPL; ++q) lds_store_f64(yw[q], yp[q]);
          wave_lds_fence();
          double atyp[CPL], axp[RPL];
          col_step(atyp, zero_c, tau);                   // tau A^T y+
#pragma unroll
          for (int q = 0; q < CPL; ++q) lds_store_f64(xw[q], xp[q]);
          wave_lds_fence();
          row_step(axp, zero_r, -sig);                   // -sig A x+
          const double ieta = 1.0 / opt_here(a.eta);
          const double itau = w * ieta, nisig = -(iw * ieta);
          // red: 0 pres^2, 1 dres^2, 2 pobj, 3 dobj, 4 sum|y| viol, 5 sum|c x|, 6 sum|dual residual| |x|
          //      (4 and 6 bound the objective error caused by the remaining infeasibility)
          double red[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
          for (int q = 0; q < CPL; ++q) {
            const double rc = c[q] - itau * atyp[q];
            // A reduced cost is absorbed as the multiplier of whichever finite bound has the matching sign (the textbook dual
            // objective: a valid lower bound).  PDLP's alternative - count it as a dual residual unless the iterate sits on that
            // bound - was measured: identical iteration counts under the per-term tests of rounds 1-2, and under the summed
            // error bound below it counts the complementarity product of such a column twice (once inside the gap, once as
            // |residual| |x|), which kept scenarios with gap = 0.72 x limit running to 31 k iterations.
            const double lbq = lb[q], ubq = ub[q];
            const double lp = is_finite(lbq) ? fmax(rc, 0.0) : 0.0;
            const double lm = is_finite(ubq) ? fmax(-rc, 0.0) : 0.0;
            const double dr_ = (rc - lp + lm) / lds_load_f64(scl_lds + 512u * q);
            red[1] = fma(dr_, dr_, red[1]);
            red[6] = fma(fabs(rc - lp + lm), fabs(xp[q]), red[6]);
            const double cx = c[q] * xp[q];
            red[2] += cx;
            red[5] += fabs(cx);
            red[3] += lp * finite_or_zero(lbq) - lm * finite_or_zero(ubq);
          }
#pragma unroll
          for (int q = 0; q < RPL; ++q) {
            const double ax_ = nisig * axp[q];
            const double rlo_q = rlo[q].get(), rhi_q = rhi[q].get();
            double viol_s = fmax(rlo_q - ax_, 0.0) + fmax(ax_ - rhi_q, 0.0);
            if constexpr (QP) {
              if (kap[q] > 0.0) {
                // soft row: no violation; (a.x - b)^2 / (2 kappa) joins the primal objective, -kappa y^2 / 2 the dual one
                const double dev = ax_ - rlo_q;
                red[2] = fma(0.5 * dev, dev / kap[q], red[2]);
                red[3] = fma(-0.5 * kap[q] * yp[q], yp[q], red[3]);
                viol_s = 0.0;
              }
            }
            const double viol = viol_s / lds_load_f64(scl_lds + 512u * (CPL + q));
            red[0] = fma(viol, viol, red[0]);
            red[4] = fma(fabs(yp[q]), viol_s, red[4]);
            red[3] += fmax(yp[q], 0.0) * finite_or_zero(rlo_q) - fmax(-yp[q], 0.0) * finite_or_zero(rhi_q);
          }
          wave_sums<7>(red);
          const double po = red[2], dobj = red[3];
          pobj.set(po);
          if (!(po == po)) { status = DSP_STATUS_NUMERICAL; break; }
          const double rp = sqrt(red[0]) / (1.0 + qn.get());
          const double rd = sqrt(red[1]) / (1.0 + cn.get());
          const double gap = fabs(po - dobj);
          const double rg = gap / (1.0 + fabs(po) + fabs(dobj));
          // Termination.  eps_obj > 0 (default): both feasibility tests AND a bound on the objective error of x+,
          //     err = |gap| + sum |y_i| viol_i + sum |dual residual_j| |x_j|  <=  eps_obj (1 + |c.x + c0|)
          // (the infeasibility-weighted sums are what the remaining infeasibilities can move the objective by).  The
          // classic relative gap |gap| / (1 + |c.x| + |dual objective|) is NOT tested beside it: c.x without the model
          // constant is ~500x the true objective here, so at eps_rel = 1e-9 it was just a second, 3x tighter copy of the gap
          // part of the bound - and the binding one for every straggler (KKT traces profiles/r02s_trace*.log: primal
          // objective within 5e-8 of the oracle and both residuals at 1e-12 from iteration ~5 k, the dual objective creeping
          // the last 2e-7 for another 50 k iterations).  Rounds 1-2 tested the three terms separately against 1e-7 each.
          bool done;
          double rho;                                           // how far the worst criterion is from its limit
          if (eps_obj > 0.0 && !waive_obj) {
            const double lim = fmax(eps_obj * (1.0 + fabs(po + c0.get())), 1e-12 * red[5]);
            const double err = gap + red[4] + red[6];
            done = rp <= eps && rd <= eps && err <= lim;
            rho = fmax(fmax(rp, rd) / eps, err / lim);
#ifdef DSP_KKT_TRACE   /* development: the KKT history of ONE scenario (tools/gpu_trace_scenario.py) */
            if (a.trace && s == a.trace_scenario && lane == 0 && ntrace < 4096) {
              double *t = a.trace + 12 * ntrace++;
              t[0] = it; t[1] = rp; t[2] = rd; t[3] = rg; t[4] = gap / lim; t[5] = red[4] / lim; t[6] = red[6] / lim;
              t[7] = w; t[8] = k; t[9] = w_lo.get(); t[10] = w_hi.get(); t[11] = po + c0.get();
            }
#endif
            // ---- near-miss zone: feasible, the error bound within 10x of its limit.  No 2x improvement of the bound for
            // polish_patience iterations means one of two things (KKT traces profiles/r02s_trace*.log, r02w_trace*.log):
            //  (a) the iterate sits on its ROUNDING floor - |dual residual| at 1e-14, row violations fluctuating around 1e-6
            //      on 1e5-kWh rows under a primal weight at its guard, the bound hovering between 1x and 6x its limit until it
            //      passes by chance.  Then the step that amplifies the noise of the noisy side is shortened 4x through the
            //      weight guard (primal noise = tau u |c|: raise w_lo; dual noise = sigma u |q|: lower w_hi) and the iteration
            //      restarts from here; at most 3 times, and only where the weight SITS at that guard (tightening it with the
            //      weight elsewhere sent 7 of 4096 QP scenarios to the iteration limit);
            //  (b) a slow drift along a nearly flat direction: both residuals at 1e-12, the primal objective already within
            //      1e-7 of the optimum, the bound stuck at a CONSTANT 2-6x its limit for 30-50 k iterations (a reduced cost
            //      of 1e-8 moving a 1e5-kWh state at constant speed, typically on objectives that are the small difference
            //      of large terms).  After 4 x polish_patience iterations of that, a scenario whose PRIMAL OBJECTIVE has not
            //      moved by more than a tenth of the limit over the whole period is accepted and FLAGGED (DSP_FLAG_OBJ_WAIVED):
            //      its certificate stands at <= 10 eps_obj, the objective itself has stopped.  (Without the objective test the
            //      acceptance let errors of 1.0e-6 - 2.6e-6 through on the 48-h batch at other check cadences - points whose
            //      objective was still sliding; accepting only up to 2 eps_obj left the drifting scenarios running to 140 k.)
            //      These were the slowest scenarios of every batch (rounds 1-2 waited for the stall logic below, which cannot
            //      fire before iteration ~11 k and needs two rounds).
            // (DSP_NEAR_RES > 1, development: let the zone reach out to that many eps_rel in the residuals for (a) - on a
            // rounding floor the primal residual itself hovers at 2-20 eps_rel.  Measured at 30 and 100: no gain in the tail
            // and 3 % of the QP scenarios end up flagged - profiles/r03a_iters.log, r03v_near_res.log.)
#ifndef DSP_NEAR_RES
#define DSP_NEAR_RES 1.0
#endif
            if (!done && a.opt.polish_patience > 0 && rp <= DSP_NEAR_RES * eps && rd <= DSP_NEAR_RES * eps && err <= 10.0 * lim) {
              const double rho_o = fmax(err / lim, fmax(rp, rd) / eps);
              if (rho_o < 0.5 * pol_best.get()) { pol_best.set(rho_o); pol_it = it; pol_po.set(po); }
              else if (it - pol_it >= 4 * a.opt.polish_patience && rp <= eps && rd <= eps && fabs(po - pol_po.get()) <= 0.1 * lim) { waive_obj = true; done = true; }
              else if (it - pol_it >= a.opt.polish_patience && !pol_tried && nboost < 3) {
                const bool primal_noise = (rp > eps || rd > eps) ? rp >= rd : gap + red[4] >= red[6];
                const double wl_ = w_lo.get(), wh_ = w_hi.get();
                if (primal_noise && w < 2.0 * wl_) { w_lo.set(wl_ * 4.0); ++nboost; boost_now = true; }
                else if (!primal_noise && 2.0 * w > wh_) { w_hi.set(wh_ * 0.25); ++nboost; boost_now = true; }
                if (boost_now) { pol_best.set(INFINITY); pol_it = it; } else pol_tried = true;
              }
            } else {
              pol_it = it; pol_tried = false;
            }
          } else {
            done = rp <= eps && rd <= eps && rg <= eps;
            rho = fmax(fmax(rp, rd), rg) / eps;
            if (waive_obj && eps_obj > 0.0 && !done) {
              // objective tests waived by the stall logic: the classic relative gap, or the error bound at 10x its limit
              const double lim = fmax(eps_obj * (1.0 + fabs(po + c0.get())), 1e-12 * red[5]);
              done = rp <= eps && rd <= eps && gap + red[4] + red[6] <= 10.0 * lim;
            }
          }
          if (done) { status = DSP_STATUS_OPTIMAL; ++it; break; }
          // the objectives drifting apart after the 8th check: an LP without a solution is suspected, the certificates are
          // evaluated at the restarts from here on (see the restart block)
          suspect = a.opt.eps_infeasible > 0.0 && rg >= 0.5 && ncheck >= 8;
          if constexpr (!CERT) {
            nsus = suspect ? nsus + 1 : 0;
            if (nsus >= 3) { status = DSP_STATUS_SUSPECT; ++it; break; }
          }
          const double gf = fmin(1.0, a.opt.kkt_gate / rho);
          gate2 = r * gf * gf;
          last_kkt = ncheck;
          DSP_PROF_ADD(2)
        }
        // ---- restart test (r0 = residual at the first check after a restart) ----------------------------------
        const bool first = !(r0 < INFINITY);
        // (ARGS_HERE: what the three tests below read, in one round trip)
        double rs_, rn_, ra_ = 0.0, js_ = 0.0;
        int warm_patience = 0, stall_rescue = 0, ray_jumps = 0, check_every_ = 0;
        if constexpr (ARGS_HERE) {
          ka = args_here();
          rs_ = DSP_OPT(ka, restart_sufficient); rn_ = DSP_OPT(ka, restart_necessary); ra_ = DSP_OPT(ka, restart_artificial);
          js_ = DSP_OPT(ka, jump_steady);
          warm_patience = DSP_OPT(ka, warm_patience); stall_rescue = DSP_OPT(ka, stall_rescue); ray_jumps = DSP_OPT(ka, ray_jumps);
          check_every_ = DSP_OPT(ka, check_every);
          asm volatile("" : "+s"(rs_), "+s"(rn_), "+s"(ra_), "+s"(js_), "+s"(warm_patience), "+s"(stall_rescue), "+s"(ray_jumps), "+s"(check_every_));
          check_every_ = check_every_ > 0 ? check_every_ : (CPL + RPL > 8 ? 32 : 16);
        } else {
          rs_ = opt_here(a.opt.restart_sufficient); rn_ = opt_here(a.opt.restart_necessary);
        }
        const double beta_s2 = rs_ * rs_, beta_n2 = rn_ * rn_;
        const bool decayed = (r <= beta_s2 * r0) || (r <= beta_n2 * r0 && r > rprev);
        const bool artificial = (double)k >= DSP_OPT_LOADED(ra_, a.opt.restart_artificial) * (double)(it - it0 + 1);
        const bool give_up_warm = warm && it >= DSP_OPT_LOADED(warm_patience, a.opt.warm_patience);
        const bool do_restart = (!first && (decayed || artificial)) || boost_now || give_up_warm;
        // no decay for >= stall_rescue iterations: the iteration sits on its rounding floor (dsp_options::stall_rescue).
        // First time, with the weight within 30x of its rounding guard: the controller has driven the weight away, reset
        // it.  From the second time on: nothing more to gain, the eps_obj tests are waived (the eps_rel tests stay).
        const bool floor_hit = do_restart && !boost_now && !decayed && DSP_OPT_LOADED(stall_rescue, a.opt.stall_rescue) > 0 && k >= DSP_OPT_LOADED(stall_rescue, a.opt.stall_rescue);
        const bool stalled = floor_hit && stalls == 0 && (w < 30.0 * w_lo.get() || 30.0 * w > w_hi.get());
        if (floor_hit && ++stalls >= 2) { waive_obj = true; gate2 = INFINITY; }
#ifdef DSP_NO_JUMP
        const bool steady = false;
#else
        // steady residual over two checks, or (chaining, ray_jumps = 2) the previous event was a jump: a landing point
        // usually lies on the next piece's ray already, so it is tested again at its first check
        if constexpr (!ARGS_HERE) js_ = opt_here(a.opt.jump_steady);
        const double steady_lo2 = (1.0 - js_) * (1.0 - js_), steady_hi2 = (1.0 + js_) * (1.0 + js_);
        const bool steady = DSP_OPT_LOADED(ray_jumps, a.opt.ray_jumps) && !do_restart && k >= jump_not_before &&
                            ((k >= 2 * DSP_OPT_LOADED(check_every_, check_every) && rprev >= steady_lo2 * r && rprev <= steady_hi2 * r) ||
                             (DSP_OPT_LOADED(ray_jumps, a.opt.ray_jumps) > 1 && lastjump && k >= DSP_OPT_LOADED(check_every_, check_every)));
#endif
        if (first) r0 = r;
        rprev = r;
        if (do_restart) {
          // the matrix values are on their way while the displacement is reduced and the weight updated (EARLY_MAT: shapes
          // whose register file has room for them next to the iterate)
          double mat_c[EARLY_MAT ? RegEll<CPL, WC>::N : 1], mat_r[EARLY_MAT ? RegEll<RPL, WR>::N : 1];
          if constexpr (EARLY_MAT) { mreg_c.fetch(P.mr_ellc, lane, mat_c); mreg_r.fetch(P.mr_ellr, lane, mat_r); }
          double dd[2] = {0.0, 0.0};
#pragma unroll
          for (int q = 0; q < CPL; ++q) { const double t = xp[q] - x0[q]; dd[0] = fma(t, t, dd[0]); }
#pragma unroll
          for (int q = 0; q < RPL; ++q) { const double t = yp[q] - y0[q]; dd[1] = fma(t, t, dd[1]); }
          wave_sums<2>(dd);
          const double w_was = w;
          if (give_up_warm) {
            // the cold point: x = clamp(0), y = 0, the automatic weight; every piece of history the controllers keep starts over
#pragma unroll
            for (int q = 0; q < CPL; ++q) xp[q] = clampd(0.0, lb[q], ub[q]);
#pragma unroll
            for (int q = 0; q < RPL; ++q) yp[q] = 0.0;
            w = w_init.get();
            warm = false; it0 = it; stalls = 0; waive_obj = false; suspect = false; nsus = 0; gate2 = 0.0; last_kkt = ncheck;
            pol_best.set(INFINITY); pol_it = it; nboost = 0; pol_tried = false;
          } else if (stalled) {
            w = sqrt(w * w_init.get());
          } else if (dd[0] > 1e-28 && dd[1] > 1e-28) {
            // log(w |dx| / |dy|) and the exponential in single precision (hardware v_log_f32 / v_exp_f32): the weight
            // is a heuristic parameter, 1e-7 relative noise on it is irrelevant and FP64 log + exp cost ~150 instructions
            const float e = __logf((float)w) + 0.5f * (__logf((float)dd[0]) - __logf((float)dd[1]));
            if constexpr (ARGS_HERE) ka = args_here();
            const float kp_ = (float)DSP_OPT_F64(pid_kp), md_ = (float)DSP_OPT_F64(max_dlog_weight);
            const float dl = fminf(fmaxf(-kp_ * e, -md_), md_);
            w *= (double)__expf(dl);
          }
          { const double wl_ = w_lo.get(); w = fmin(fmax(w, wl_), fmax(w_hi.get(), wl_)); }
          if constexpr (EARLY_MAT) {
            if (w != w_was) { DSP_SET_SCALARS() mreg_c.rescale(tau, mat_c); mreg_r.rescale(-sig, mat_r); }
          } else {
            if (w != w_was) DSP_SET_STEPS()
          }
#pragma unroll
          for (int q = 0; q < CPL; ++q) { x[q] = xp[q]; x0[q] = xp[q]; }
#pragma unroll
          for (int q = 0; q < RPL; ++q) { y[q] = yp[q]; y0[q] = yp[q]; }
          k = 0; r0 = INFINITY; rprev = INFINITY; jump_not_before = 0;
          lastjump = false;
          moved = true;
          DSP_PROF_ADD(3)
          // ---- infeasibility / unboundedness certificates (dsp_options::eps_infeasible) ---------------------------------------
          // An LP without a solution has no fixed point: T(z) - z tends to a ray (dx, dy), one of the objectives runs away and the
          // relative gap goes to 1.  On the bidding LPs of every workload the gap is below 1/2 by the 8th check (lab:
          // tools/infeas_lab.py, no test at all on 4 x 64 feasible scenarios), so feasible batches pay one comparison per KKT
          // test.  dy, with the signs its rows cannot take removed, is tested as a FARKAS RAY (reduced costs -A'dy absorbed by
          // finite column bounds, bound value > 0); dx, clipped to the recession cone of the column bounds, as a direction of
          // UNBOUNDED descent (c.dx < 0, A dx in the recession cone of the rows).  Both are proofs up to the tolerance whatever
          // the iterate; scaled space (diagonal scalings map the cones onto themselves).  Soft rows (QP) admit no multiplier ray
          // and count as equalities for the recession cone.  Lab: a 24-h bidding LP with 10 x the battery as initial charge is
          // certified at iteration 192, unbounded variants at 0.8 - 2.5 k (five of six; the rest of the LP keeps converging
          // underneath the ray, and its movement counts as violation until it has).
          // Evaluated HERE, right after a restart: anchor and iterate coincide, so a third of the per-scenario state is dead and the
          // two extra products fit without new spills on the common paths (in the KKT block they cost the 48-h kernel 10 %).
          if constexpr (CERT) if (suspect) {
            DSP_PDHG_STEP()                                // (x+, y+) = T(x, y) from the restart point: the displacement the certificates use
            const double ieta = 1.0 / opt_here(a.eta);
            const double itau = w * ieta, nisig = -(iw * ieta);
            double atyp[CPL], axp[RPL];
            double rr[6] = {0, 0, 0, 0, 0, 0};   // 0 |dual residual of the ray|^2, 1 its bound value, 2 |bounds|^2, 3 |recession violation|^2, 4 c.d, 5 |c|^2
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
              const double dy = yp[q] - y[q];
              const double rlo_q = rlo[q].get(), rhi_q = rhi[q].get();
              double yc = (is_finite(rlo_q) ? fmax(dy, 0.0) : 0.0) - (is_finite(rhi_q) ? fmax(-dy, 0.0) : 0.0);
              if constexpr (QP) { if (kap[q] > 0.0) yc = 0.0; }
              lds_store_f64(yw[q], yc);
              rr[1] += fmax(yc, 0.0) * finite_or_zero(rlo_q) - fmax(-yc, 0.0) * finite_or_zero(rhi_q);
              const double big = fmax(fabs(finite_or_zero(rlo_q)), fabs(finite_or_zero(rhi_q)));
              rr[2] = fma(big, big, rr[2]);
            }
            wave_lds_fence();
            col_step(atyp, zero_c, tau);                   // tau A^T (cleaned dy)
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
              const double lbq = lb[q], ubq = ub[q];
              const bool fl = is_finite(lbq), fu = is_finite(ubq);
              const double rc = -(itau * atyp[q]);
              const double lp = fl ? fmax(rc, 0.0) : 0.0, lm = fu ? fmax(-rc, 0.0) : 0.0;
              const double res = rc - lp + lm;
              rr[0] = fma(res, res, rr[0]);
              rr[1] += lp * finite_or_zero(lbq) - lm * finite_or_zero(ubq);
              const double lf = finite_or_zero(lbq), uf = finite_or_zero(ubq);
              rr[2] += lf * lf + uf * uf;
              const double dx = xp[q] - x[q];
              const double d = (fl && fu) ? 0.0 : fl ? fmax(dx, 0.0) : fu ? fmin(dx, 0.0) : dx;
              lds_store_f64(xw[q], d);
              rr[4] = fma(c[q], d, rr[4]);
              rr[5] = fma(c[q], c[q], rr[5]);
            }
            wave_lds_fence();
            row_step(axp, zero_r, -sig);                   // -sig A (clipped dx)
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
              const double ad = nisig * axp[q];
              const double rv = (is_finite(rlo[q].get()) ? fmax(-ad, 0.0) : 0.0) + (is_finite(rhi[q].get()) ? fmax(ad, 0.0) : 0.0);
              rr[3] = fma(rv, rv, rr[3]);
            }
            wave_sums<6>(rr);
            const double ei = a.opt.eps_infeasible;
            if (rr[1] > 0.0 && sqrt(rr[0]) * (1.0 + sqrt(rr[2])) <= ei * rr[1]) { status = DSP_STATUS_PRIMAL_INFEASIBLE; ++it; break; }
            if (rr[4] < 0.0 && sqrt(rr[3]) * (1.0 + sqrt(rr[5])) <= ei * -rr[4]) { status = DSP_STATUS_DUAL_INFEASIBLE; ++it; break; }
          }
        } else if (steady) {
          // ---- ray jump: second application of T from (x+, y+), translation test, ratio test ------------------
          double x2[CPL], y2[RPL];
#pragma unroll
          for (int q = 0; q < RPL; ++q) lds_store_f64(yw[q], yp[q]);
          wave_lds_fence();
          double tt[2] = {0.0, 0.0};       // |v2 - v1|^2_w, |v2|^2_w
          double gx1[CPL], gy1[RPL];
#pragma unroll
          for (int q = 0; q < CPL; ++q) gx1[q] = fma(-tau, c[q], xp[q]);
          col_step(gx1, gx1, tau);       // x+ - tau (c - A^T y+)
#pragma unroll
          for (int q = 0; q < CPL; ++q) {
            x2[q] = clampd(gx1[q], lb[q], ub[q]);
            lds_store_f64(xw[q], 2.0 * x2[q] - xp[q]);
            const double v1 = xp[q] - x[q], v2 = x2[q] - xp[q];
            tt[0] = fma(w * (v2 - v1), v2 - v1, tt[0]);
            tt[1] = fma(w * v2, v2, tt[1]);
          }
          wave_lds_fence();
          row_step(gy1, yp, -sig);       // y+ - sig A (2 x2 - x+)
#pragma unroll
          for (int q = 0; q < RPL; ++q) {
            y2[q] = gy1[q] - clampd(gy1[q], ylo[q], yhi[q]);
            if constexpr (QP) y2[q] *= srow[q];
            const double v1 = yp[q] - y[q], v2 = y2[q] - yp[q];
            tt[0] = fma(iw * (v2 - v1), v2 - v1, tt[0]);
            tt[1] = fma(iw * v2, v2, tt[1]);
          }
          wave_sums<2>(tt);
          // the ratio test (one FP64 division per owned element + a wave-min) only for rays that pass the translation
          // test: about one attempt in ten
          double alpha = 0.0;
          if constexpr (ARGS_HERE) ka = args_here();
          const double jt_ = DSP_OPT_F64(jump_tol);
          if (tt[1] > 0.0 && tt[0] <= jt_ * jt_ * tt[1]) {
            // the unprojected points of the FIRST application, recomputed (bit-identical to what the step above had)
            double g0x[CPL], g0y[RPL];
#pragma unroll
            for (int q = 0; q < RPL; ++q) lds_store_f64(yw[q], y[q]);
            wave_lds_fence();
#pragma unroll
            for (int q = 0; q < CPL; ++q) g0x[q] = fma(-tau, c[q], x[q]);
            col_step(g0x, g0x, tau);
#pragma unroll
            for (int q = 0; q < CPL; ++q) lds_store_f64(xw[q], 2.0 * xp[q] - x[q]);
            wave_lds_fence();
            row_step(g0y, y, -sig);
            alpha = INFINITY;
#pragma unroll
            for (int q = 0; q < CPL; ++q) alpha = fmin(alpha, steps_to_break(gx1[q], gx1[q] - g0x[q], lb[q], ub[q]));
#pragma unroll
            for (int q = 0; q < RPL; ++q)
              alpha = fmin(alpha, steps_to_break(-gy1[q], g0y[q] - gy1[q], sig * rlo[q].get(), sig * rhi[q].get()));
            alpha = wave_min(alpha);
          }
          // a ray that is too short to be worth an anchor reset reaches its breakpoint by itself in alpha steps: no
          // point in testing again before that
          if constexpr (ARGS_HERE) ka = args_here();
          if (alpha >= DSP_OPT_HERE(jump_min) && alpha < DSP_OPT_HERE(jump_rel) * (double)k) jump_not_before = k + (int)fmin(alpha, 1e6);
          if (alpha >= DSP_OPT_HERE(jump_min) && alpha >= DSP_OPT_HERE(jump_rel) * (double)k && alpha < 1e200) {
            const double al = floor(alpha) - 1.0;
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
              const double xn = clampd(x2[q] + al * (x2[q] - xp[q]), lb[q], ub[q]);
              x[q] = xn; x0[q] = xn; xp[q] = xn;
            }
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
              const double yn = y2[q] + al * (y2[q] - yp[q]);
              y[q] = yn; y0[q] = yn; yp[q] = yn;
            }
            k = 0; r0 = INFINITY; rprev = INFINITY; jump_not_before = 0;
            ++njump;
            lastjump = true;
            moved = true;
          }
          DSP_PROF_ADD(4)
        }
      }
      ++it;
      if (!moved) DSP_HALPERN_STEP(DSP_ANCHOR_WEIGHT())
      DSP_PROF_ADD(5)
    }
#undef DSP_OPT_HERE
#undef DSP_OPT_LOADED
#undef DSP_OPT_F64
#undef DSP_PDHG_STEP
#undef DSP_SET_STEPS
#undef DSP_SET_SCALARS
#undef DSP_SET_MATRICES
#undef DSP_HALPERN_STEP
#undef DSP_ANCHOR_WEIGHT

    DSP_TRACE("[trace] store status=%d it=%d\n", status, it);
    if constexpr (!MATREG) if (a.skip_solved == 3) {
      // re-certification: only a CERTIFIED optimum replaces the point the earlier pass accepted; the work is accounted either way
      if (lane == 0 && b.iters) b.iters[s] = it + it_base;
      if (status != DSP_STATUS_OPTIMAL || waive_obj) continue;
      if (lane == 0) atomicSub(a.suspects + 2, 1);
    }
    // ---- store the scenario's result (unscaled) ----------------------------------------------------------
    if (status != DSP_STATUS_OPTIMAL) {
      double po = 0.0;
#pragma unroll
      for (int q = 0; q < CPL; ++q) po = fma(c[q], xp[q], po);
      if constexpr (QP) {
#pragma unroll
        for (int q = 0; q < CPL; ++q) lds_store_f64(xw[q], xp[q]);
        wave_lds_fence();
        double axq[RPL];
        row_step(axq, zero_r, -sig);                     // -sig A x+
        const double ieta = 1.0 / opt_here(a.eta);
#pragma unroll
        for (int q = 0; q < RPL; ++q)
          if (kap[q] > 0.0) { const double dev = -(iw * ieta) * axq[q] - rlo[q].get(); po = fma(0.5 * dev, dev / kap[q], po); }
      }
      pobj.set(wave_sum(po));
    }
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      const int j = col_id(q);
      if (j >= 0) b.x[(size_t)s * n + j] = xp[q] * P.col_scale[j];
    }
    DSP_TRACE("[trace] x stored %p\n", (void *)b.x);
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
      const int i = row_id(q);
      if (i >= 0) b.y[(size_t)s * m + i] = yp[q] * P.row_scale[i];
    }
    DSP_TRACE("[trace] y stored %p obj %p status %p iters %p jumps %p pw %p queue %p\n", (void *)b.y, (void *)b.obj, (void *)b.status, (void *)b.iters, (void *)b.jumps, (void *)b.primal_weight, (void *)a.queue);
    if (lane == 0) {
      b.obj[s] = pobj.get();
      b.status[s] = status;
      if (b.iters) b.iters[s] = it + it_base;
      if (status == DSP_STATUS_SUSPECT) atomicAdd(a.suspects, 1);
      if (waive_obj && status == DSP_STATUS_OPTIMAL) atomicAdd(a.suspects + 2, 1);      // count of flagged scenarios (re-certification pass)
#ifdef DSP_CLOCKS
      iters_done += it;
#endif
      if (b.jumps) b.jumps[s] = njump;
      if (b.flags) b.flags[s] = (waive_obj && status == DSP_STATUS_OPTIMAL ? DSP_FLAG_OBJ_WAIVED : 0) | (stalls > 0 ? DSP_FLAG_STALL_RESCUE : 0) | (nboost > 0 ? DSP_FLAG_POLISH : 0);
      if (b.primal_weight) b.primal_weight[s] = w;
    }
    DSP_TRACE("[trace] scalars stored\n");
  }
#ifdef DSP_PROF
  if (lane == 0 && (blockIdx.x % 397) == 0 && prof_n[0] > 0)
    printf("[prof] block %d: hot %lld cyc / %lld segments | check base %lld / %lld | kkt %lld / %lld | restart %lld / %lld | jump test %lld / %lld | tail %lld / %lld\n",
           (int)blockIdx.x, prof_c[0], prof_n[0], prof_c[1], prof_n[1], prof_c[2], prof_n[2], prof_c[3], prof_n[3], prof_c[4], prof_n[4], prof_c[5], prof_n[5]);
#endif
#ifdef DSP_CLOCKS
  if (lane == 0 && (blockIdx.x % 509) == 0 && iters_done > 0) {
    const long long dc = clock64() - clk0, dw = wall_clock64() - wall0;
    printf("[clocks] block %d: %.2f ms, shader clock %.0f MHz, %lld iterations, %.0f shader cycles / iteration\n",
           (int)blockIdx.x, dw * 1e-5, 100.0 * (double)dc / (double)dw, iters_done, (double)dc / (double)iters_done);
  }
#endif
}

// ---- streaming SpMV step: AX = A X, ATY = A^T Y with vectors in HBM --------------------------------------
// One scenario per wave; the (unscaled) ELL matrix is staged into LDS once per workgroup; each wave streams its
// x (coalesced) into its LDS exchange buffer, forms the row products from LDS and writes them coalesced.
// Algorithmic HBM bytes per scenario: 2*8*(n+m)  (read x,y; write Ax, A^T y).  The results are written once and never read
// back by this kernel: NON-TEMPORAL stores (no L2 write-allocate).  BASELINE.md section 3 configuration (T = 48, B = 4096,
// 41 MB): 10.4 -> 8.8 us = 4.66 TB/s = 58 % of the 8 TB/s peak (target <= 10.2 us); metric batch (T = 24, 20.6 MB) 6.3 -> 5.8
// us = 44 %; 131 072 scenarios 60 -> 66 % (T = 24), 70 -> 72 % (T = 48).  Non-temporal LOADS as well were measured worse
// (48 h: 9.3 us), 16-wave blocks (half the matrix staging) gain nothing on top (profiles/r03k, r03l, r03n_spmv_*.log).
template <int CPL, int RPL, bool LONG>
__global__ void __launch_bounds__(1024) spmv_step_kernel(SpmvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const DeviceProblem &P = a.P;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  Entry *ellc = reinterpret_cast<Entry *>(smem);
  Entry *ellr = ellc + P.ellc_entries;
  Entry *tailc = ellr + P.ellr_entries;
  Entry *tailr = tailc + P.tailc_entries;
  char *wave_buf = reinterpret_cast<char *>(tailr + P.tailr_entries);
  stage_entries(ellc, P.ellc_unscaled, P.ellc_entries);
  stage_entries(ellr, P.ellr_unscaled, P.ellr_entries);
  stage_entries(tailc, P.tailc_unscaled, P.tailc_entries);
  stage_entries(tailr, P.tailr_unscaled, P.tailr_entries);
  const int n = P.n, m = P.m;
  const int waves_total = gridDim.x * a.waves_per_block;
  int s = blockIdx.x * a.waves_per_block + wave;
  // first scenario's vectors are in flight while the matrix is staged
  double xr[CPL], yr[RPL];
  if (s < a.B) {
#pragma unroll
    for (int q = 0; q < CPL; ++q) { const int j = lane + 64 * q; xr[q] = (j < n) ? a.X[(size_t)s * n + j] : 0.0; }
#pragma unroll
    for (int q = 0; q < RPL; ++q) { const int i = lane + 64 * q; yr[q] = (i < m) ? a.Y[(size_t)s * m + i] : 0.0; }
  }
  __syncthreads();
  char *xb = wave_buf + (size_t)wave * (P.n_pad + P.m_pad) * 8;
  char *yb = xb + (size_t)P.n_pad * 8;
  double *xbl = reinterpret_cast<double *>(xb) + lane;
  double *ybl = reinterpret_cast<double *>(yb) + lane;
  for (; s < a.B; s += waves_total) {
#pragma unroll
    for (int q = 0; q < CPL; ++q) xbl[64 * q] = xr[q];
#pragma unroll
    for (int q = 0; q < RPL; ++q) ybl[64 * q] = yr[q];
    wave_lds_fence();
    // prefetch the next scenario of this wave
    const int sn = s + waves_total;
    if (sn < a.B) {
#pragma unroll
      for (int q = 0; q < CPL; ++q) { const int j = lane + 64 * q; xr[q] = (j < n) ? a.X[(size_t)sn * n + j] : 0.0; }
#pragma unroll
      for (int q = 0; q < RPL; ++q) { const int i = lane + 64 * q; yr[q] = (i < m) ? a.Y[(size_t)sn * m + i] : 0.0; }
    }
    double axv[RPL], atyv[CPL];
    ell_product<RPL, LONG>(axv, ellr, P.Wr, xb, lane, P.long_r, tailr);
    ell_product<CPL, LONG>(atyv, ellc, P.Wc, yb, lane, P.long_c, tailc);
#pragma unroll
    for (int q = 0; q < RPL; ++q) { const int i = lane + 64 * q; if (i < m) __builtin_nontemporal_store(axv[q], &a.AX[(size_t)s * m + i]); }
#pragma unroll
    for (int q = 0; q < CPL; ++q) { const int j = lane + 64 * q; if (j < n) __builtin_nontemporal_store(atyv[q], &a.ATY[(size_t)s * n + j]); }
    wave_lds_fence();
  }
}

#ifdef __HIPCC_RTC__      /* run-time compiled code objects carry the layout token they were compiled with (dsp_device.hpp) */
}  // namespace dsp
extern "C" __device__ __attribute__((used)) const unsigned long long dsp_rtc_layout_token = dsp::kSolveArgsToken;
namespace dsp {
#endif

#if !defined(__HIPCC_RTC__) && !defined(DSP_KERNELS_ONLY)     /* everything below is host code (DSP_KERNELS_ONLY: development TUs that instantiate single kernels, tools/kernel_resources.sh) */
// ---- launch tables ------------------------------------------------------------------------------------------
// Register-resident-matrix specialisations exist for the shapes of the reference's flowsheets at the benchmark
// horizons (cols/lane, rows/lane, ELL width of A^T, ELL width of A, long vectors): everything else runs the generic
// LDS-matrix kernel.  wind+battery 24 h, nuclear 24 h / 48 h, wind+PEM 48 h (shared capacity column = long vector).
// X(cols/lane, rows/lane, per-slot widths of A^T (4 bits each, slot 0 lowest), per-slot widths of A, long vectors,
//   c/lb/ub in LDS)
#define DSP_MATREG_SHAPES(X)                                                                                  \
  X(4, 2, 0x1133u, 0x44u, false)         /* wind+battery 24 h */                                              \
  X(3, 2, 0x122u, 0x24u, false)          /* nuclear 24 h      */                                              \
  X(5, 3, 0x11222u, 0x234u, false)       /* nuclear 48 h      */                                              \
  X(4, 3, 0x1122u, 0x233u, true)         /* wind+PEM 48 h     */                                              \
  X(7, 4, 0x1112333u, 0x2444u, false)    /* wind+battery 48 h */                                              \
  X(1, 1, 0x3u, 0x4u, false)             /* wind+battery real-time bids and tracking, 4 h */                  \
  X(1, 1, 0x4u, 0x3u, false)             /* wind+PEM real-time bids, 4 h */                                   \
  X(2, 1, 0x12u, 0x4u, false)            /* nuclear real-time bids, 12 h */                                  \
  X(2, 1, 0x13u, 0x4u, false)            /* wind+battery 12 h */                                              \
  X(5, 3, 0x11333u, 0x344u, false)       /* wind+battery 36 h */                                              \
  X(2, 2, 0x12u, 0x23u, true)            /* wind+PEM 24 h     */                                              \
  X(3, 2, 0x122u, 0x33u, true)           /* wind+PEM 36 h     */                                              \
  X(4, 2, 0x1122u, 0x34u, false)         /* nuclear 36 h      */                                              \
  /* PADDED specialisations (every slot 4 entries wide, zero-filled): any LP without long vectors whose columns and  \
     rows have <= 4 entries gets a register-resident matrix even when no tight shape was compiled for it (other       \
     horizons, perturbed flowsheets): ~1.3-1.5x the gathers and FMAs of a tight shape, still well ahead of the       \
     LDS-matrix kernel */                                                                                             \
  X(1, 1, 0x4u, 0x4u, false)                                                                                          \
  X(2, 1, 0x44u, 0x4u, false)                                                                                         \
  X(2, 2, 0x44u, 0x44u, false)                                                                                        \
  X(3, 2, 0x444u, 0x44u, false)                                                                                       \
  X(4, 2, 0x4444u, 0x44u, false)                                                                                      \
  X(4, 3, 0x4444u, 0x444u, false)                                                                                     \
  X(5, 3, 0x44444u, 0x444u, false)

// QP instantiations (soft rows, dsp_batch::row_compliance) of the register-resident kernel: the ramp-cost variant of the
// metric LP (BASELINE config 5) + the padded shapes.  Every other QP without long vectors runs the generic QP kernel.
#define DSP_MATREG_QP_SHAPES(X)                                                                               \
  X(4, 3, 0x1135u, 0x244u, false)        /* wind+battery 24 h + quadratic ramp cost (23 soft rows) */          \
  X(2, 2, 0x44u, 0x44u, false)                                                                                \
  X(3, 2, 0x444u, 0x44u, false)                                                                               \
  X(4, 2, 0x4444u, 0x44u, false)                                                                              \
  X(4, 3, 0x4444u, 0x444u, false)                                                                             \
  X(5, 3, 0x44444u, 0x444u, false)

// 0 = no specialisation, 1 = register-resident matrix
int matreg_available(int cpl, int rpl, unsigned wc, unsigned wr, bool lng, bool qp) {
#ifdef DSP_NO_MATREG
  return 0;
#else
#define DSP_X(C, R, WC_, WR_, L) if (cpl == C && rpl == R && wc == WC_ && wr == WR_ && lng == L) return 1;
  if (qp) { DSP_MATREG_QP_SHAPES(DSP_X) }
  else { DSP_MATREG_SHAPES(DSP_X) }
#undef DSP_X
  return 0;
#endif
}

static const void *matreg_fn(int cpl, int rpl, unsigned wc, unsigned wr, bool lng, bool qp) {
#ifndef DSP_NO_MATREG
#define DSP_X(C, R, WC_, WR_, L)                                                            \
  if (cpl == C && rpl == R && wc == WC_ && wr == WR_ && lng == L)                           \
    return reinterpret_cast<const void *>(&pdlp_solve_kernel<C, R, L, WC_, WR_>);
  if (!qp) { DSP_MATREG_SHAPES(DSP_X) }
#undef DSP_X
#define DSP_X(C, R, WC_, WR_, L)                                                            \
  if (cpl == C && rpl == R && wc == WC_ && wr == WR_ && lng == L)                           \
    return reinterpret_cast<const void *>(&pdlp_solve_kernel<C, R, L, WC_, WR_, true>);
  if (qp) { DSP_MATREG_QP_SHAPES(DSP_X) }
#undef DSP_X
#endif
  return nullptr;
}

template <int CPL, int RPL>
static const void *generic_fn(bool lng, bool qp) {
  if (qp) return lng ? nullptr : reinterpret_cast<const void *>(&pdlp_solve_kernel<CPL, RPL, false, 0u, 0u, true>);
  return lng ? reinterpret_cast<const void *>(&pdlp_solve_kernel<CPL, RPL, true, 0u, 0u>)
             : reinterpret_cast<const void *>(&pdlp_solve_kernel<CPL, RPL, false, 0u, 0u>);
}

// the LIGHT instantiation of the generic kernel that follows the first pass `first`, nullptr where the first pass is no three-wave kernel
static const void *light_fn(int cpl, int rpl, const SolveArgs &first) {
#ifndef DSP_NO_MATREG
  const bool lng = first.P.long_c.count > 0 || first.P.long_r.count > 0;
  if (!first.matreg || !three_waves_first_pass(cpl, rpl, first.P.mr_wc_pack, first.P.mr_wr_pack, lng, first.qp != 0)) return nullptr;
  static_assert(three_waves_first_pass(4, 2, 0x1133u, 0x44u, false, false), "the light instantiation below follows this first pass");
  if (cpl == 4 && rpl == 2) return reinterpret_cast<const void *>(&pdlp_solve_kernel<4, 2, false, 0u, 0u, false, true>);
#endif
  return nullptr;
}
// resident one-wave blocks per CU of the light follow-up kernel behind the first pass `first`; 0: there is none (or it does not fit)
int light_followup_blocks(int cpl, int rpl, const SolveArgs &first, size_t lds) {
  const void *fn = light_fn(cpl, rpl, first);
  int nb = 0;
  if (!fn || hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 64, lds) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return nb;
}
// a follow-up pass `a` (matreg = 0) in blocks of one wave; `first`: the first pass it follows
hipError_t launch_solve_light(int cpl, int rpl, const SolveArgs &first, const SolveArgs &a, int grid, size_t lds, hipStream_t st) {
  const void *fn = light_fn(cpl, rpl, first);
  if (!fn || a.matreg || a.waves_per_block != 1) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  SolveArgs args = a;
  void *params[] = {&args};
  return hipLaunchKernel(fn, dim3(grid), dim3(64), params, lds, st);
}

template <int CPL, int RPL>
static hipError_t launch_solve_t(const SolveArgs &a, dim3 grid, dim3 block, size_t lds, hipStream_t st) {
  const bool lng = a.P.long_c.count > 0 || a.P.long_r.count > 0;
  const void *fn = a.matreg ? matreg_fn(CPL, RPL, a.P.mr_wc_pack, a.P.mr_wr_pack, lng, a.qp != 0) : generic_fn<CPL, RPL>(lng, a.qp != 0);
  if (!fn) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  SolveArgs args = a;
  void *params[] = {&args};
  return hipLaunchKernel(fn, grid, block, params, lds, st);
}
template <int CPL, int RPL>
static hipError_t launch_spmv_t(const SpmvArgs &a, dim3 grid, dim3 block, size_t lds, hipStream_t st) {
  const bool lng = a.P.long_c.count > 0 || a.P.long_r.count > 0;
  const void *fn = lng ? reinterpret_cast<const void *>(&spmv_step_kernel<CPL, RPL, true>)
                       : reinterpret_cast<const void *>(&spmv_step_kernel<CPL, RPL, false>);
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  if (lng) hipLaunchKernelGGL((spmv_step_kernel<CPL, RPL, true>), grid, block, lds, st, a);
  else hipLaunchKernelGGL((spmv_step_kernel<CPL, RPL, false>), grid, block, lds, st, a);
  return hipGetLastError();
}

#ifdef DSP_SINGLE_VARIANT   /* development: instantiate only <4,2> for -save-temps inspection */
#define DSP_FOR_CPL(F) if (cpl == 4 && rpl == 2) return F<4, 2>(a, grid, block, lds, st); return hipErrorInvalidValue;
#else
#define DSP_FOR_RPL(F, C)                                                                                   \
  switch (rpl) {                                                                                            \
    case 1: return F<C, 1>(a, grid, block, lds, st);                                                        \
    case 2: return F<C, 2>(a, grid, block, lds, st);                                                        \
    case 3: return F<C, 3>(a, grid, block, lds, st);                                                        \
    case 4: return F<C, 4>(a, grid, block, lds, st);                                                        \
    case 6: return F<C, 6>(a, grid, block, lds, st);                                                        \
    default: return hipErrorInvalidValue;                                                                   \
  }
#define DSP_FOR_CPL(F)                                                                                      \
  switch (cpl) {                                                                                            \
    case 1: DSP_FOR_RPL(F, 1)                                                                               \
    case 2: DSP_FOR_RPL(F, 2)                                                                               \
    case 3: DSP_FOR_RPL(F, 3)                                                                               \
    case 4: DSP_FOR_RPL(F, 4)                                                                               \
    case 5: DSP_FOR_RPL(F, 5)                                                                               \
    case 7: DSP_FOR_RPL(F, 7)                                                                               \
    case 10: DSP_FOR_RPL(F, 10)                                                                             \
    default: return hipErrorInvalidValue;                                                                   \
  }
#endif

hipError_t launch_solve(int cpl, int rpl, const SolveArgs &a, dim3 grid, dim3 block, size_t lds, hipStream_t st) {
  DSP_FOR_CPL(launch_solve_t)
}

// resident blocks per CU of the solve kernel for a block shape (register- and LDS-limited): the "launch" is dry
template <int CPL, int RPL>
static hipError_t occupancy_solve_t(const SolveArgs &a, dim3 grid, dim3 block, size_t lds, hipStream_t) {
  const bool lng = a.P.long_c.count > 0 || a.P.long_r.count > 0;
  const void *fn = a.matreg ? matreg_fn(CPL, RPL, a.P.mr_wc_pack, a.P.mr_wr_pack, lng, a.qp != 0) : generic_fn<CPL, RPL>(lng, a.qp != 0);
  if (!fn) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  int nb = 0;
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, (int)block.x, lds);
  *reinterpret_cast<int *>(a.queue) = nb;      // host pointer smuggled through the (unused) queue field
  (void)grid;
  return e;
}
hipError_t occupancy_solve(int cpl, int rpl, const SolveArgs &a0, int block_threads, size_t lds, int *blocks_per_cu) {
  SolveArgs a = a0;
  a.queue = blocks_per_cu;
  dim3 grid(1), block(block_threads);
  hipStream_t st = nullptr;
  DSP_FOR_CPL(occupancy_solve_t)
}
// The streaming SpMV step is a MEASUREMENT kernel (the HBM roofline of one A x + one A^T y with the vectors in HBM; no
// solve calls it): instantiated for the shapes of the benchmark workloads only (scenarios.WORKLOADS: wind + battery 24 / 48 h, nuclear
// 24 / 48 h, wind + PEM 48 h and its shared capacity column), hipErrorInvalidValue for any other LP.
hipError_t launch_spmv(int cpl, int rpl, const SpmvArgs &a, dim3 grid, dim3 block, size_t lds, hipStream_t st) {
  if (cpl == 4 && rpl == 2) return launch_spmv_t<4, 2>(a, grid, block, lds, st);
  if (cpl == 7 && rpl == 4) return launch_spmv_t<7, 4>(a, grid, block, lds, st);
  if (cpl == 3 && rpl == 2) return launch_spmv_t<3, 2>(a, grid, block, lds, st);
  if (cpl == 5 && rpl == 3) return launch_spmv_t<5, 3>(a, grid, block, lds, st);
  if (cpl == 4 && rpl == 3) return launch_spmv_t<4, 3>(a, grid, block, lds, st);
  return hipErrorInvalidValue;
}

#endif   // __HIPCC_RTC__

}  // namespace dsp
