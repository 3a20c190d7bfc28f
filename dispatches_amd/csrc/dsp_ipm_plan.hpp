// dsp_ipm_plan.hpp — host-side plan of the interior-point form (dsp_ipm.hip): whether an LP is TIME-BANDED, and if it is, what the
// kernels read of its scaled matrix.  No HIP here: ipm_create uploads what ipm_plan_build returns, and tests/ipm_plan_harness.cpp
// compiles this file with g++ (tests/test_ipm_plan_cpu.py).
//
// In the natural (period-major) row order a column of a time-banded LP touches rows that lie close together.  A column whose rows span
// more than kIpmSpan is WIDE (design variables, periodic conditions; kIpmMaxK at most): it leaves the band and enters the normal equations
// through Sherman-Morrison-Woodbury.  The largest span of the other (NARROW) columns is the half-bandwidth of  A_narrow Theta A_narrow',
// rounded up to W = 6 or 8.  The plan holds
//   the band's product lists  B(t, t - k) = sum bval * theta[bcol]  (k = 0 .. W; k_ipm_assemble),
//   the scaled matrix as two ELLs - rows over all columns, narrow columns over their rows - of fixed widths (multiples of four: the
//     kernels take the entries four at a time; padding: index 0, value 0) and the wide columns as a CSR with ascending rows,
//   the geometry of the time-parallel walks (dsp_ipm_seq.hpp: IpmParts).
// Not of the kind (ipm_plan_build returns false; the PDHG forms are the general path): fewer than 64 rows, more than kIpmMaxK wide columns,
// a half-bandwidth above kIpmMaxW, or more than 16 entries in a row, in a narrow column or in a product list.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "dsp_ipm_seq.hpp"
#include "dsp_prepare.hpp"

namespace dsp {

constexpr int kIpmMaxW = 8, kIpmMaxK = 4, kIpmSpan = 16;
constexpr int kIpmMinRows = 64, kIpmMaxWidth = 16;

struct IpmHostPlan {
  int n = 0, m = 0, W = 0, K = 0;
  int rw = 0, cw = 0, bw = 0;               // entries per row (all columns), per NARROW column, products per band entry
  std::vector<uint8_t> wide;                // [n] 0 = narrow, k + 1 = wide column k
  std::vector<int32_t> wide_col;            // [K]
  std::vector<int32_t> rcol, crow;          // [m][rw], [n][cw] (wide columns: empty here)
  std::vector<double> rval, cval;
  std::vector<int32_t> wptr, wrow;          // the wide columns' entries: CSR over k, rows ascending (k_ipm_wide_rhs searches them by row)
  std::vector<double> wval;
  std::vector<int32_t> bcol;                // [m][W + 1][bw]
  std::vector<double> bval;
  IpmParts parts{};
};

// last row - first row of column j (a row of AT); -1: the column is empty
inline int ipm_col_span(const HostCSR &AT, int j) {
  if (AT.ptr[j + 1] == AT.ptr[j]) return -1;
  int lo = AT.idx[AT.ptr[j]], hi = lo;
  for (int p = AT.ptr[j]; p < AT.ptr[j + 1]; ++p) { lo = std::min(lo, (int)AT.idx[p]); hi = std::max(hi, (int)AT.idx[p]); }
  return hi - lo;
}

inline int ipm_round4(int w) { return (w + 3) / 4 * 4; }

// B(t, t - k) = sum over the narrow columns j of rows t and t - k: a_tj a_(t-k)j theta_j.  Returns the longest list (unrounded); fills
// bcol / bval only if that fits kIpmMaxWidth.
inline int ipm_band_products(const HostCSR &A, const std::vector<uint8_t> &wide, int W, std::vector<int32_t> &bcol, std::vector<double> &bval) {
  const int m = A.m, W1 = W + 1;
  std::vector<std::vector<std::pair<int32_t, double>>> prod((size_t)m * W1);
  int longest = 1;
  for (int t = 0; t < m; ++t)
    for (int k = 0; k < W1 && k <= t; ++k) {
      const int r2 = t - k;
      auto &pl = prod[(size_t)t * W1 + k];
      for (int p = A.ptr[t]; p < A.ptr[t + 1]; ++p) {
        const int j = A.idx[p];
        if (wide[j]) continue;
        for (int p2 = A.ptr[r2]; p2 < A.ptr[r2 + 1]; ++p2)
          if (A.idx[p2] == j) pl.push_back({j, A.val[p] * A.val[p2]});
      }
      longest = std::max(longest, (int)pl.size());
    }
  if (longest > kIpmMaxWidth) return longest;
  const int bw = ipm_round4(longest);
  bcol.assign((size_t)m * W1 * bw, 0);
  bval.assign((size_t)m * W1 * bw, 0.0);
  for (size_t e = 0; e < prod.size(); ++e)
    for (size_t q = 0; q < prod[e].size(); ++q) { bcol[e * bw + q] = prod[e][q].first; bval[e * bw + q] = prod[e][q].second; }
  return longest;
}

// the longest row of M among those `skip` leaves in (null: all), at least 1
inline int ipm_longest_row(const HostCSR &M, const std::vector<uint8_t> *skip) {
  int w = 1;
  for (int i = 0; i < M.m; ++i) if (!skip || !(*skip)[i]) w = std::max(w, M.ptr[i + 1] - M.ptr[i]);
  return w;
}
// ELL of fixed width `w` of the rows of M (the rows `skip` marks stay empty)
inline void ipm_ell(const HostCSR &M, const std::vector<uint8_t> *skip, int w, std::vector<int32_t> &idx, std::vector<double> &val) {
  idx.assign((size_t)M.m * w, 0);
  val.assign((size_t)M.m * w, 0.0);
  for (int i = 0; i < M.m; ++i)
    if (!skip || !(*skip)[i])
      for (int p = M.ptr[i], q = 0; p < M.ptr[i + 1]; ++p, ++q) { idx[(size_t)i * w + q] = M.idx[p]; val[(size_t)i * w + q] = M.val[p]; }
}

inline void ipm_wide_csr(const HostCSR &AT, IpmHostPlan &H) {
  H.wptr.assign(1, 0);
  for (int j : H.wide_col) {
    std::vector<std::pair<int32_t, double>> ent;
    for (int p = AT.ptr[j]; p < AT.ptr[j + 1]; ++p) ent.push_back({(int32_t)AT.idx[p], AT.val[p]});
    std::sort(ent.begin(), ent.end());
    for (const auto &en : ent) { H.wrow.push_back(en.first); H.wval.push_back(en.second); }
    H.wptr.push_back((int32_t)H.wrow.size());
  }
}

// m rows in partitions of Lp rows (Lp >= m: one partition, the sequential walks)
inline IpmParts ipm_partition_rows(int m, int W, int Lp) {
  IpmParts g{};
  g.m = m; g.W = W; g.P = 1; g.Lp = m;
  int parts = (m + Lp - 1) / Lp;
  if (parts > 1 && m - (parts - 1) * Lp < 2 * W + 1) parts -= 1;         // a short tail joins the partition before it
  if (parts >= 2) { g.P = parts; g.Lp = Lp; }
  return g;
}
// time-parallel form: partitions of >= 256 rows, 64 at most (the reduced system's 63 sequential blocks then weigh about as much as a
// partition's 820 rows at T = 8736); `requested` > 0 (DSP_IPM_PARTS; 1: the sequential walks) asks for any count the rows allow
inline IpmParts ipm_partition(int m, int W, int requested) {
  const int want = requested > 0 ? requested : std::min(64, m / 256);
  return ipm_partition_rows(m, W, want >= 2 ? std::max((m + want - 1) / want, 4 * W) : m);
}

// The plan of the scaled matrix A (AT: its transpose) with `requested_parts` partitions (0: automatic); false: not a time-banded LP.
inline bool ipm_plan_build(const HostCSR &A, const HostCSR &AT, int requested_parts, IpmHostPlan &H) {
  H = IpmHostPlan{};
  const int n = A.n, m = A.m;
  if (m < kIpmMinRows) return false;
  H.n = n; H.m = m;
  H.wide.assign(n, 0);
  int band = 0;
  for (int j = 0; j < n; ++j) {
    const int span = ipm_col_span(AT, j);
    if (span <= kIpmSpan) { band = std::max(band, span); continue; }
    if ((int)H.wide_col.size() == kIpmMaxK) return false;
    H.wide_col.push_back(j);
    H.wide[j] = (uint8_t)H.wide_col.size();
  }
  if (band > kIpmMaxW) return false;
  H.K = (int)H.wide_col.size();
  H.W = band <= 6 ? 6 : 8;
  const int bw = ipm_band_products(A, H.wide, H.W, H.bcol, H.bval);
  const int rw = ipm_longest_row(A, nullptr), cw = ipm_longest_row(AT, &H.wide);
  if (rw > kIpmMaxWidth || cw > kIpmMaxWidth || bw > kIpmMaxWidth) return false;      // not the sparse time-banded kind after all
  H.rw = ipm_round4(rw); H.cw = ipm_round4(cw); H.bw = ipm_round4(bw);
  ipm_ell(A, nullptr, H.rw, H.rcol, H.rval);
  ipm_ell(AT, &H.wide, H.cw, H.crow, H.cval);
  ipm_wide_csr(AT, H);
  H.parts = ipm_partition(m, H.W, requested_parts);
  return true;
}

}  // namespace dsp
