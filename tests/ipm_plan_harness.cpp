// CPU harness of the interior-point form's plan (test infrastructure): csrc/dsp_ipm_plan.hpp builds, from a scaled matrix and its
// transpose, everything the kernels of csrc/dsp_ipm.hip read of the LP's structure - or refuses the LP.  This program makes a small
// time-banded matrix, runs the planner and checks what it returns against the matrix itself, densely.
// Usage: ipm_plan_harness T rows_per_period band wide seed [parts [row_entries [Lp]]]  ->  one JSON line.
//   m = T * rows_per_period rows.  Narrow column j (one per row) has an entry in row j and one in row j + d, d random in 1 .. band
//   (column 0: d = band, so that the half-bandwidth is reached); `wide` further columns touch every (m / 5)-th row or so.
//   parts: the partition count asked for (0: automatic).  row_entries > 0: row m / 2 is filled up to that many entries by columns
//   of its own.  Lp > 0: also print the geometry of partitions of Lp rows (ipm_partition_rows).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../dispatches_amd/csrc/dsp_ipm_plan.hpp"

using namespace dsp;

int main(int argc, char **argv) {
  if (argc < 6) { fprintf(stderr, "usage: %s T rows_per_period band wide seed [parts [row_entries [Lp]]]\n", argv[0]); return 2; }
  const int T = atoi(argv[1]), R = atoi(argv[2]), band = atoi(argv[3]), K = atoi(argv[4]);
  const unsigned seed = (unsigned)atoi(argv[5]);
  const int parts = argc > 6 ? atoi(argv[6]) : 0, row_entries = argc > 7 ? atoi(argv[7]) : 0, Lp = argc > 8 ? atoi(argv[8]) : 0;
  const int m = T * R;
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.5, 2.0);
  auto value = [&]() { return (rng() & 1 ? 1.0 : -1.0) * U(rng); };
  // rows as lists of (column, value), columns in ascending order within a row
  std::vector<std::vector<std::pair<int, double>>> rows(m);
  int n = 0;
  for (int j = 0; j < m; ++j, ++n) {
    rows[j].push_back({n, value()});
    const int d = j == 0 ? band : 1 + (int)(rng() % (unsigned)std::max(band, 1));
    if (band > 0 && j + d < m) rows[j + d].push_back({n, value()});
  }
  for (int k = 0; k < K; ++k, ++n)
    for (int i = (int)(rng() % 7u); i < m; i += std::max(m / 5, 1) + k) rows[i].push_back({n, value()});
  while (row_entries > 0 && (int)rows[m / 2].size() < row_entries) rows[m / 2].push_back({n++, value()});
  HostCSR A;
  A.m = m; A.n = n;
  A.ptr.assign(1, 0);
  for (int i = 0; i < m; ++i) {
    std::sort(rows[i].begin(), rows[i].end());
    for (const auto &en : rows[i]) { A.idx.push_back(en.first); A.val.push_back(en.second); }
    A.ptr.push_back((int32_t)A.idx.size());
  }
  const HostCSR AT = transpose(A);

  IpmHostPlan H;
  const bool ok = ipm_plan_build(A, AT, parts, H);
  printf("{\"ok\": %d, \"m\": %d, \"n\": %d", ok ? 1 : 0, m, n);
  if (Lp > 0) { const IpmParts g = ipm_partition_rows(m, band <= 6 ? 6 : 8, Lp); printf(", \"rows_P\": %d, \"rows_Lp\": %d", g.P, g.Lp); }
  if (!ok) { printf("}\n"); return 0; }
  const int W = H.W, W1 = W + 1;
  printf(", \"W\": %d, \"K\": %d, \"rw\": %d, \"cw\": %d, \"bw\": %d, \"P\": %d, \"Lp\": %d", W, H.K, H.rw, H.cw, H.bw, H.parts.P, H.parts.Lp);

  // the band's product lists against  A_narrow diag(theta) A_narrow'  computed densely
  std::vector<double> theta(n), x(n), y(m);
  for (double &v : theta) v = U(rng);
  for (double &v : x) v = value();
  for (double &v : y) v = value();
  std::vector<double> N((size_t)m * m, 0.0);
  for (int j = 0; j < n; ++j)
    if (!H.wide[j])
      for (int p = AT.ptr[j]; p < AT.ptr[j + 1]; ++p)
        for (int p2 = AT.ptr[j]; p2 < AT.ptr[j + 1]; ++p2) N[(size_t)AT.idx[p] * m + AT.idx[p2]] += AT.val[p] * theta[j] * AT.val[p2];
  double band_err = 0.0, beyond = 0.0, scale = 0.0;
  for (double v : N) scale = std::max(scale, std::fabs(v));
  for (int t = 0; t < m; ++t)
    for (int s = 0; s < m; ++s)
      if (std::abs(t - s) > W) beyond = std::max(beyond, std::fabs(N[(size_t)t * m + s]));
  int pad_ok = 1;
  for (int t = 0; t < m; ++t)
    for (int k = 0; k < W1; ++k) {
      double sum = 0.0;
      for (int q = 0; q < H.bw; ++q) {
        const size_t e = ((size_t)t * W1 + k) * H.bw + q;
        sum += H.bval[e] * theta[H.bcol[e]];
        if (H.bval[e] == 0.0 && H.bcol[e] != 0) pad_ok = 0;
        if (H.bval[e] != 0.0 && H.wide[H.bcol[e]]) pad_ok = 0;                      // (a wide column has no business in the band)
      }
      const double ref = t - k >= 0 ? N[(size_t)t * m + (t - k)] : 0.0;
      band_err = std::max(band_err, std::fabs(sum - ref) / scale);
    }
  // the row ELL reproduces A x; the narrow columns' ELL and the wide columns' CSR reproduce A' y
  double ax_err = 0.0, aty_err = 0.0;
  for (int i = 0; i < m; ++i) {
    double ref = 0.0, ell = 0.0;
    for (int p = A.ptr[i]; p < A.ptr[i + 1]; ++p) ref += A.val[p] * x[A.idx[p]];
    for (int q = 0; q < H.rw; ++q) {
      ell += H.rval[(size_t)i * H.rw + q] * x[H.rcol[(size_t)i * H.rw + q]];
      if (q >= A.ptr[i + 1] - A.ptr[i] && (H.rcol[(size_t)i * H.rw + q] != 0 || H.rval[(size_t)i * H.rw + q] != 0.0)) pad_ok = 0;
    }
    ax_err = std::max(ax_err, std::fabs(ell - ref));
  }
  int wide_sorted = 1, wide_seen = 0;
  for (int j = 0; j < n; ++j) {
    double ref = 0.0, got = 0.0;
    for (int p = AT.ptr[j]; p < AT.ptr[j + 1]; ++p) ref += AT.val[p] * y[AT.idx[p]];
    const int len = H.wide[j] ? 0 : AT.ptr[j + 1] - AT.ptr[j];
    for (int q = 0; q < H.cw; ++q) {
      got += H.cval[(size_t)j * H.cw + q] * y[H.crow[(size_t)j * H.cw + q]];
      if (q >= len && (H.crow[(size_t)j * H.cw + q] != 0 || H.cval[(size_t)j * H.cw + q] != 0.0)) pad_ok = 0;
    }
    if (H.wide[j]) {
      const int k = H.wide[j] - 1;
      if (k >= H.K || H.wide_col[k] != j) wide_sorted = 0;
      ++wide_seen;
      for (int p = H.wptr[k]; p < H.wptr[k + 1]; ++p) {
        got += H.wval[p] * y[H.wrow[p]];
        if (p > H.wptr[k] && H.wrow[p] <= H.wrow[p - 1]) wide_sorted = 0;
      }
    }
    aty_err = std::max(aty_err, std::fabs(got - ref));
  }
  if (wide_seen != H.K || (int)H.wptr.size() != H.K + 1) wide_sorted = 0;
  printf(", \"band_err\": %.3e, \"beyond_band\": %.3e, \"ax_err\": %.3e, \"aty_err\": %.3e, \"padding_ok\": %d, \"wide_ok\": %d}\n", band_err, beyond,
         ax_err, aty_err, pad_ok, wide_sorted);
  return 0;
}
