// eg3d_fund_core.h — the arithmetic of the fundamental-matrix estimator (row N4), stated ONCE for the host and the device.
//
// host/fundamental.cpp (eg3d_host_estimate_fundamental) is the plain, sequential use of these functions and thereby the
// DEFINITION of the result; the K12 kernels (eg3d_k12_fundamental.hip, eg3d_estimate_fundamental) call the same functions
// and must return the same bits. It restates host/fmatrix.cpp (eg3d_host_estimate_F), per ORDERED pair (i, j), i != j:
//
//   common points   the points seen from both views in ascending id; a repeated view id in a track counts once; the
//                   position is the LAST listed observation with that view id; entries with a view id outside [0, V)
//                   are ignored; fewer than kMinCommon points: no matrix (F_valid = 0, F = 0).
//   sampling        `iterations` samples of 8 distinct indices from ONE SplitMix64 stream per pair, started at
//                   stream_seed(rng_seed, i * V + j); below(n) = next() % n; a duplicate index is drawn again. The stream
//                   is sequential over the iterations; a degenerate sample consumes its draws and is skipped.
//   fit             the normalised 8-point fit of fmatrix.cpp's eight_point, every sum in the order written here; the
//                   cyclic Jacobi keeps its 60 sweeps and its two thresholds; rank 2, denormalisation and the scaling by
//                   1 / F[8] (or the Frobenius norm) as there.
//   residual        the larger of the two squared point-to-line distances; a non-finite value becomes kHuge.
//   selection       the median is the n/2-th smallest (from zero); the smallest median wins, the earlier iteration on a tie.
//   inliers, refit  residual <= max(sigma^2, 1e-12), sigma = 2.5 * 1.4826 * (1 + 5 / (n - 8 + (n == 8))) * sqrt(best median);
//                   the refit runs on the inliers in ascending index and is kept only if its median is <= the best.
//
// The ONE deliberate difference from fmatrix.cpp: the distance in the Hartley normalisation is sqrt(dx*dx + dy*dy), not
// std::hypot. glibc >= 2.35 resolves hypot at load time to an FMA or a non-FMA body; the two need not agree in the last
// bit, and one flipped `median < best` comparison selects another sample. sqrt of a sum of two products is exact
// everywhere under the project's arithmetic contract: -ffp-contract=off on both sides, correctly rounded FP64 sqrt and
// division, no reordering of any sum.
//
// Everything here indexes its small matrices with compile-time constants only (the rotations are a template recursion),
// so that on the device both 9 x 9 matrices of a fit stay in registers: an index the compiler cannot resolve would send
// the whole matrix to private memory.
#pragma once
#include "eg3d_dev_geom.h"

#if defined(__clang__)
#define EG3D_FUND_UNROLL _Pragma("unroll")
#else
#define EG3D_FUND_UNROLL
#endif

namespace eg3d {
namespace fund {

constexpr int kMinCommon = 10;  // MIN_CORRESPONDENCES_AMOUNT, geometric_utilities.cpp:752
constexpr int kSample = 8;
constexpr uint32_t kDefaultIterations = 300;  // as fmatrix.cpp
constexpr double kHuge = 1e300;
constexpr double kSqrt2 = 1.4142135623730951;  // the double nearest to sqrt(2)

struct Rng {  // SplitMix64
  uint64_t s;
  EG3D_HD uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  EG3D_HD uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};
EG3D_HD uint64_t stream_seed(uint64_t rng_seed, uint64_t ij) { return rng_seed ^ (0x9E3779B97F4A7C15ull * (ij + 1)); }

// 8 distinct indices below n (n >= 8)
EG3D_HD_FLAT void draw_sample(Rng& rng, uint32_t n, uint32_t (&idx)[kSample]) {
  EG3D_FUND_UNROLL
  for (int k = 0; k < kSample; k++) {
    uint32_t c;
    bool dup;
    do {
      c = rng.below(n);
      dup = false;
      EG3D_FUND_UNROLL
      for (int m = 0; m < k; m++) dup |= idx[m] == c;
    } while (dup);
    idx[k] = c;
  }
}

EG3D_HD bool finite_f64(double x) {
  uint64_t b;
  __builtin_memcpy(&b, &x, 8);
  return (b & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

// ---- cyclic Jacobi eigen-decomposition of a symmetric N x N matrix: eigenvalues on the diagonal of a, eigenvectors in
// the columns of v. Both triangles of a are rotated, as in fmatrix.cpp (the 2 x 2 block of a rotation does not stay
// symmetric to the last bit, and the lower triangle feeds later rotations).
template <int N, int P, int Q>
EG3D_HD_FLAT void jacobi_rotate(double (&a)[N][N], double (&v)[N][N]) {
  if (__builtin_fabs(a[P][Q]) < 1e-300) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * a[P][Q]);
  const double t = (theta >= 0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + EG3D_SQRT(theta * theta + 1.0));
  const double c = 1.0 / EG3D_SQRT(t * t + 1.0), s = t * c;
  EG3D_FUND_UNROLL
  for (int k = 0; k < N; k++) {
    const double akp = a[k][P], akq = a[k][Q];
    a[k][P] = c * akp - s * akq;
    a[k][Q] = s * akp + c * akq;
  }
  EG3D_FUND_UNROLL
  for (int k = 0; k < N; k++) {
    const double apk = a[P][k], aqk = a[Q][k];
    a[P][k] = c * apk - s * aqk;
    a[Q][k] = s * apk + c * aqk;
  }
  EG3D_FUND_UNROLL
  for (int k = 0; k < N; k++) {
    const double vkp = v[k][P], vkq = v[k][Q];
    v[k][P] = c * vkp - s * vkq;
    v[k][Q] = s * vkp + c * vkq;
  }
}
// the rotations of one sweep, (0,1), (0,2) .. (N-2,N-1), from (P, Q) on
template <int N, int P, int Q>
EG3D_HD_FLAT void jacobi_sweep(double (&a)[N][N], double (&v)[N][N]) {
  jacobi_rotate<N, P, Q>(a, v);
  if constexpr (Q + 1 < N)
    jacobi_sweep<N, P, Q + 1>(a, v);
  else if constexpr (P + 2 < N)
    jacobi_sweep<N, P + 1, P + 2>(a, v);
}
template <int N>
EG3D_HD_FLAT void jacobi_eigen(double (&a)[N][N], double (&v)[N][N]) {
  EG3D_FUND_UNROLL
  for (int i = 0; i < N; i++) {
    EG3D_FUND_UNROLL
    for (int j = 0; j < N; j++) v[i][j] = i == j ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0, diag = 0;
    EG3D_FUND_UNROLL
    for (int p = 0; p < N; p++) {
      diag += a[p][p] * a[p][p];
      EG3D_FUND_UNROLL
      for (int q = p + 1; q < N; q++) off += a[p][q] * a[p][q];
    }
    if (off <= 1e-30 * diag) break;  // (per lane on the device: a lane that is done does not rotate again)
    jacobi_sweep<N, 0, 1>(a, v);
  }
}
// column `lo` of v, lo = the first index of the smallest diagonal entry of a (tracked as a value: no run-time index)
template <int N>
EG3D_HD_FLAT void smallest_eigenvector(const double (&a)[N][N], const double (&v)[N][N], double (&out)[N]) {
  double least = a[0][0];
  EG3D_FUND_UNROLL
  for (int k = 0; k < N; k++) out[k] = v[k][0];
  EG3D_FUND_UNROLL
  for (int c = 1; c < N; c++)
    if (a[c][c] < least) {
      least = a[c][c];
      EG3D_FUND_UNROLL
      for (int k = 0; k < N; k++) out[k] = v[k][c];
    }
}

// ---- the normalised 8-point fit ---------------------------------------------------------------------------------------------
struct Corr {  // one correspondence: (x1, y1) on view i, (x2, y2) on view j
  double x1, y1, x2, y2;
};
// Hartley normalisation: centroid to the origin, mean distance sqrt(2). T = [[s,0,-s cx],[0,s,-s cy],[0,0,1]].
struct Norm {
  double s, cx, cy;
};
EG3D_HD double norm_dist(double dx, double dy) { return EG3D_SQRT(dx * dx + dy * dy); }  // NOT hypot: see the head of the file
EG3D_HD double norm_scale(double mean_dist) { return mean_dist > 1e-12 ? kSqrt2 / mean_dist : 1.0; }
// entry a of the row r = {x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1} of a normalised correspondence, as a product
// u[a / 3] * w[a % 3] over u = (x2, y2, 1), w = (x1, y1, 1): a product with 1.0 is exact, so this is r[a] to the bit
EG3D_HD double row_entry(int a, double x1, double y1, double x2, double y2) {
  const int ua = a / 3, wa = a % 3;
  const double u = ua == 0 ? x2 : ua == 1 ? y2 : 1.0;
  const double w = wa == 0 ? x1 : wa == 1 ? y1 : 1.0;
  return u * w;
}

// The two normalisations and the 9 x 9 normal matrix A = sum over k of r_k r_k', k = 0 .. n-1 in this order; get(k) is the
// k-th correspondence of the fit.
template <class Get>
EG3D_HD_FLAT void build_normal(const Get& get, int n, Norm& n1, Norm& n2, double (&A)[9][9]) {
  double cx1 = 0, cy1 = 0, cx2 = 0, cy2 = 0;
  for (int k = 0; k < n; k++) {
    const Corr p = get(k);
    cx1 += p.x1;
    cy1 += p.y1;
    cx2 += p.x2;
    cy2 += p.y2;
  }
  cx1 /= n;
  cy1 /= n;
  cx2 /= n;
  cy2 /= n;
  double d1 = 0, d2 = 0;
  for (int k = 0; k < n; k++) {
    const Corr p = get(k);
    d1 += norm_dist(p.x1 - cx1, p.y1 - cy1);
    d2 += norm_dist(p.x2 - cx2, p.y2 - cy2);
  }
  d1 /= n;
  d2 /= n;
  n1 = Norm{norm_scale(d1), cx1, cy1};
  n2 = Norm{norm_scale(d2), cx2, cy2};
  EG3D_FUND_UNROLL
  for (int a = 0; a < 9; a++) {
    EG3D_FUND_UNROLL
    for (int b = 0; b < 9; b++) A[a][b] = 0;
  }
  for (int k = 0; k < n; k++) {
    const Corr p = get(k);
    const double x1 = (p.x1 - n1.cx) * n1.s, y1 = (p.y1 - n1.cy) * n1.s;
    const double x2 = (p.x2 - n2.cx) * n2.s, y2 = (p.y2 - n2.cy) * n2.s;
    const double r[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
    EG3D_FUND_UNROLL
    for (int a = 0; a < 9; a++) {
      EG3D_FUND_UNROLL
      for (int b = 0; b < 9; b++) A[a][b] += r[a] * r[b];
    }
  }
}

// From the normal matrix (destroyed) to F: x2' F x1 = 0, rank 2 enforced. False on a degenerate fit.
EG3D_HD_FLAT bool solve_normal(double (&A)[9][9], const Norm& n1, const Norm& n2, double (&F)[9]) {
  double V[9][9];
  jacobi_eigen<9>(A, V);
  double f[9];
  smallest_eigenvector<9>(A, V, f);
  double Fn[3][3];
  EG3D_FUND_UNROLL
  for (int a = 0; a < 9; a++) Fn[a / 3][a % 3] = f[a];
  // rank 2: remove the component along the right singular vector of the smallest singular value
  double G[3][3], W[3][3], w[3];
  EG3D_FUND_UNROLL
  for (int a = 0; a < 3; a++) {
    EG3D_FUND_UNROLL
    for (int b = 0; b < 3; b++) {
      double t = 0;
      EG3D_FUND_UNROLL
      for (int k = 0; k < 3; k++) t += Fn[k][a] * Fn[k][b];
      G[a][b] = t;
    }
  }
  jacobi_eigen<3>(G, W);
  smallest_eigenvector<3>(G, W, w);
  double Fv[3];
  EG3D_FUND_UNROLL
  for (int a = 0; a < 3; a++) Fv[a] = Fn[a][0] * w[0] + Fn[a][1] * w[1] + Fn[a][2] * w[2];
  EG3D_FUND_UNROLL
  for (int a = 0; a < 3; a++) {
    EG3D_FUND_UNROLL
    for (int b = 0; b < 3; b++) Fn[a][b] -= Fv[a] * w[b];
  }
  // denormalise: F = T2' Fn T1
  const double T1[3][3] = {{n1.s, 0, -n1.s * n1.cx}, {0, n1.s, -n1.s * n1.cy}, {0, 0, 1}};
  const double T2[3][3] = {{n2.s, 0, -n2.s * n2.cx}, {0, n2.s, -n2.s * n2.cy}, {0, 0, 1}};
  double M[3][3];
  EG3D_FUND_UNROLL
  for (int a = 0; a < 3; a++) {
    EG3D_FUND_UNROLL
    for (int b = 0; b < 3; b++) {
      double t = 0;
      EG3D_FUND_UNROLL
      for (int k = 0; k < 3; k++) t += Fn[a][k] * T1[k][b];
      M[a][b] = t;
    }
  }
  double nrm = 0;
  EG3D_FUND_UNROLL
  for (int a = 0; a < 3; a++) {
    EG3D_FUND_UNROLL
    for (int b = 0; b < 3; b++) {
      double t = 0;
      EG3D_FUND_UNROLL
      for (int k = 0; k < 3; k++) t += T2[k][a] * M[k][b];
      F[3 * a + b] = t;
      nrm += t * t;
    }
  }
  if (!(nrm > 0) || !finite_f64(nrm)) return false;
  // scale as OpenCV reports it (F33 = 1) when that entry is not tiny, unit Frobenius norm otherwise
  const double sc = __builtin_fabs(F[8]) > 1e-12 * EG3D_SQRT(nrm) ? 1.0 / F[8] : 1.0 / EG3D_SQRT(nrm);
  EG3D_FUND_UNROLL
  for (int a = 0; a < 9; a++) F[a] *= sc;
  return true;
}

template <class Get>
EG3D_HD_FLAT bool eight_point(const Get& get, int n, double (&F)[9]) {
  Norm n1, n2;
  double A[9][9];
  build_normal(get, n, n1, n2, A);
  return solve_normal(A, n1, n2, F);
}

// larger of the two squared point-to-epipolar-line distances; >= +0, or kHuge: its bit pattern orders as an unsigned integer
EG3D_HD double residual(const double (&F)[9], const Corr& p) {
  const double l2x = F[0] * p.x1 + F[1] * p.y1 + F[2], l2y = F[3] * p.x1 + F[4] * p.y1 + F[5], l2c = F[6] * p.x1 + F[7] * p.y1 + F[8];
  const double e2 = p.x2 * l2x + p.y2 * l2y + l2c;
  const double d2 = e2 * e2 / (l2x * l2x + l2y * l2y);
  const double l1x = F[0] * p.x2 + F[3] * p.y2 + F[6], l1y = F[1] * p.x2 + F[4] * p.y2 + F[7], l1c = F[2] * p.x2 + F[5] * p.y2 + F[8];
  const double e1 = p.x1 * l1x + p.y1 * l1y + l1c;
  const double d1 = e1 * e1 / (l1x * l1x + l1y * l1y);
  const double d = d1 > d2 ? d1 : d2;
  return finite_f64(d) ? d : kHuge;
}

// the inlier threshold from the best median
EG3D_HD double inlier_threshold(double best_med, int n) {
  const double sigma = 2.5 * 1.4826 * (1.0 + 5.0 / (n - kSample + (n == kSample))) * EG3D_SQRT(best_med);
  const double s2 = sigma * sigma;
  return s2 < 1e-12 ? 1e-12 : s2;
}

}  // namespace fund
}  // namespace eg3d
