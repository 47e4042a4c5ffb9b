// transform.cpp — the similarity fit to known camera centres and its application to points and cameras
// (include/eg3d_host_transform.h states every formula and its order; this file is its plain, sequential statement).
// The fit is FP64 and unpinned (Eigen is not available to the project); everything after the conversion of T is FP32 in
// the evaluation order of the glm the reference vendors.
#include <cmath>
#include <cstring>
#include <fstream>

#include "../../include/eg3d_host_transform.h"

namespace {

constexpr int kSweeps = 30;
constexpr double kPairEps = 2.220446049250313e-16;  // 2^-52
constexpr double kRankTol = 1e-12;
constexpr double kDegenerate = 1e-28;

inline bool finite3(const double* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

double det3(const double m[3][3]) {
  return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])) +
         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// a = U diag(d) V^T, one-sided Jacobi on the columns of a (3 x 3); d descending; U completed to a right-handed orthonormal
// basis where a singular value counts as zero. Returns the rank.
int svd3(const double a_in[3][3], double U[3][3], double d[3], double V[3][3]) {
  double A[3][3], W[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  memcpy(A, a_in, sizeof(A));
  static const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2};
  for (int sweep = 0; sweep < kSweeps; sweep++) {
    bool rotated = false;
    for (int k = 0; k < 3; k++) {
      const int p = P[k], q = Q[k];
      const double alpha = (A[0][p] * A[0][p] + A[1][p] * A[1][p]) + A[2][p] * A[2][p];
      const double beta = (A[0][q] * A[0][q] + A[1][q] * A[1][q]) + A[2][q] * A[2][q];
      const double gamma = (A[0][p] * A[0][q] + A[1][p] * A[1][q]) + A[2][p] * A[2][q];
      if (gamma == 0.0 || std::fabs(gamma) <= kPairEps * std::sqrt(alpha * beta)) continue;
      rotated = true;
      const double zeta = (beta - alpha) / (2.0 * gamma);
      const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
      for (int r = 0; r < 3; r++) {
        const double ap = A[r][p], aq = A[r][q];
        A[r][p] = c * ap - s * aq;
        A[r][q] = s * ap + c * aq;
        const double vp = W[r][p], vq = W[r][q];
        W[r][p] = c * vp - s * vq;
        W[r][q] = s * vp + c * vq;
      }
    }
    if (!rotated) break;
  }
  double n[3];
  for (int j = 0; j < 3; j++) n[j] = std::sqrt((A[0][j] * A[0][j] + A[1][j] * A[1][j]) + A[2][j] * A[2][j]);
  int ord[3] = {0, 1, 2};  // insertion sort, descending, stable
  for (int i = 1; i < 3; i++)
    for (int j = i; j > 0 && n[ord[j]] > n[ord[j - 1]]; j--) {
      const int x = ord[j];
      ord[j] = ord[j - 1];
      ord[j - 1] = x;
    }
  int rank = 0;
  for (int j = 0; j < 3; j++) {
    d[j] = n[ord[j]];
    for (int r = 0; r < 3; r++) V[r][j] = W[r][ord[j]];
    if (d[j] > kRankTol * d[0] && d[j] > 0.0) {
      for (int r = 0; r < 3; r++) U[r][j] = A[r][ord[j]] / d[j];
      rank = j + 1;  // (descending: the columns above the tolerance come first)
    }
  }
  if (rank == 0) {
    for (int r = 0; r < 3; r++)
      for (int j = 0; j < 3; j++) U[r][j] = r == j ? 1.0 : 0.0;
    return 0;
  }
  if (rank == 1) {  // any unit vector orthogonal to u0: start from the axis u0 leans on least
    int e = 0;
    for (int r = 1; r < 3; r++)
      if (std::fabs(U[r][0]) < std::fabs(U[e][0])) e = r;
    double w[3], dot = U[e][0];
    for (int r = 0; r < 3; r++) w[r] = (r == e ? 1.0 : 0.0) - dot * U[r][0];
    const double len = std::sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    for (int r = 0; r < 3; r++) U[r][1] = w[r] / len;
  }
  if (rank <= 2) {  // u2 = +-(u0 x u1), with the sign of det(V): det(U) det(V) > 0, no reflection is reported for a plane
    const double sgn = det3(V) < 0.0 ? -1.0 : 1.0;
    U[0][2] = sgn * (U[1][0] * U[2][1] - U[2][0] * U[1][1]);
    U[1][2] = sgn * (U[2][0] * U[0][1] - U[0][0] * U[2][1]);
    U[2][2] = sgn * (U[0][0] * U[1][1] - U[1][0] * U[0][1]);
  }
  return rank;
}

struct Mat4 {
  float m[4][4];
};
inline Mat4 to_f32(const double* T) {
  Mat4 M;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) M.m[i][j] = (float)T[4 * i + j];
  return M;
}

// transform_3d_point (:152-155)
inline void point(const Mat4& M, const float* p, float* out) {
  const float x = p[0], y = p[1], z = p[2], w = 1.0f;
  float h[4];
  for (int j = 0; j < 4; j++) h[j] = ((M.m[j][0] * x + M.m[j][1] * y) + M.m[j][2] * z) + M.m[j][3] * w;
  out[0] = h[0] / h[3];
  out[1] = h[1] / h[3];
  out[2] = h[2] / h[3];
}

// glm::detail::compute_inverse (type_mat4x4.inl:37-92), m[i][j] as glm indexes
Mat4 inverse(const Mat4& a) {
  const float(*m)[4] = a.m;
  const float c00 = m[2][2] * m[3][3] - m[3][2] * m[2][3], c02 = m[1][2] * m[3][3] - m[3][2] * m[1][3],
              c03 = m[1][2] * m[2][3] - m[2][2] * m[1][3];
  const float c04 = m[2][1] * m[3][3] - m[3][1] * m[2][3], c06 = m[1][1] * m[3][3] - m[3][1] * m[1][3],
              c07 = m[1][1] * m[2][3] - m[2][1] * m[1][3];
  const float c08 = m[2][1] * m[3][2] - m[3][1] * m[2][2], c10 = m[1][1] * m[3][2] - m[3][1] * m[1][2],
              c11 = m[1][1] * m[2][2] - m[2][1] * m[1][2];
  const float c12 = m[2][0] * m[3][3] - m[3][0] * m[2][3], c14 = m[1][0] * m[3][3] - m[3][0] * m[1][3],
              c15 = m[1][0] * m[2][3] - m[2][0] * m[1][3];
  const float c16 = m[2][0] * m[3][2] - m[3][0] * m[2][2], c18 = m[1][0] * m[3][2] - m[3][0] * m[1][2],
              c19 = m[1][0] * m[2][2] - m[2][0] * m[1][2];
  const float c20 = m[2][0] * m[3][1] - m[3][0] * m[2][1], c22 = m[1][0] * m[3][1] - m[3][0] * m[1][1],
              c23 = m[1][0] * m[2][1] - m[2][0] * m[1][1];
  const float f0[4] = {c00, c00, c02, c03}, f1[4] = {c04, c04, c06, c07}, f2[4] = {c08, c08, c10, c11};
  const float f3[4] = {c12, c12, c14, c15}, f4[4] = {c16, c16, c18, c19}, f5[4] = {c20, c20, c22, c23};
  const float v0[4] = {m[1][0], m[0][0], m[0][0], m[0][0]}, v1[4] = {m[1][1], m[0][1], m[0][1], m[0][1]};
  const float v2[4] = {m[1][2], m[0][2], m[0][2], m[0][2]}, v3[4] = {m[1][3], m[0][3], m[0][3], m[0][3]};
  const float sa[4] = {1.0f, -1.0f, 1.0f, -1.0f}, sb[4] = {-1.0f, 1.0f, -1.0f, 1.0f};
  Mat4 inv;
  for (int k = 0; k < 4; k++) {
    inv.m[0][k] = ((v1[k] * f0[k] - v2[k] * f1[k]) + v3[k] * f2[k]) * sa[k];
    inv.m[1][k] = ((v0[k] * f0[k] - v2[k] * f3[k]) + v3[k] * f4[k]) * sb[k];
    inv.m[2][k] = ((v0[k] * f1[k] - v1[k] * f3[k]) + v3[k] * f5[k]) * sa[k];
    inv.m[3][k] = ((v0[k] * f2[k] - v1[k] * f4[k]) + v2[k] * f5[k]) * sb[k];
  }
  const float d0 = m[0][0] * inv.m[0][0], d1 = m[0][1] * inv.m[1][0], d2 = m[0][2] * inv.m[2][0], d3 = m[0][3] * inv.m[3][0];
  const float dot = (d0 + d1) + (d2 + d3);
  const float one_over_det = 1.0f / dot;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) inv.m[i][j] = inv.m[i][j] * one_over_det;
  return inv;
}

// glm's a * b (type_mat4x4.inl:686-704): column i of the result is a's columns weighted by b[i][.]
Mat4 mul(const Mat4& a, const Mat4& b) {
  Mat4 r;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++)
      r.m[i][j] = ((a.m[0][j] * b.m[i][0] + a.m[1][j] * b.m[i][1]) + a.m[2][j] * b.m[i][2]) + a.m[3][j] * b.m[i][3];
  return r;
}

inline bool is_null(const float* R, const float* C) {
  for (int k = 0; k < 3; k++)
    if (!(C[k] == 0.0f)) return false;
  for (int k = 0; k < 9; k++)
    if (!(R[k] == 0.0f)) return false;
  return true;
}

}  // namespace

extern "C" int eg3d_host_read_camera_poses(const char* path, int n_cameras, double* out) {
  if (!path || n_cameras < 0 || (n_cameras && !out)) return EG3D_TRANSFORM_ERR_ARG;
  std::ifstream f(path);
  if (!f) return EG3D_TRANSFORM_ERR_FILE;
  for (int i = 0; i < 3 * n_cameras; i++) {
    double v;
    if (!(f >> v)) return EG3D_TRANSFORM_ERR_SHORT;
    out[i] = v;
  }
  return EG3D_TRANSFORM_OK;
}

extern "C" int eg3d_host_null_cameras(int n, const float* R9, const float* C3, uint8_t* mask_out) {
  if (n < 0 || (n && (!R9 || !C3 || !mask_out))) return EG3D_TRANSFORM_ERR_ARG;
  for (int i = 0; i < n; i++) mask_out[i] = is_null(R9 + 9 * i, C3 + 3 * i) ? 1 : 0;
  return EG3D_TRANSFORM_OK;
}

extern "C" int eg3d_host_similarity_fit(int n, const double* src, const double* dst, const uint8_t* null_mask, double* T,
                                        eg3d_similarity_stats* stats) {
  if (n < 0 || !T || (n && (!src || !dst))) return EG3D_TRANSFORM_ERR_ARG;
  if (stats && stats->struct_size < sizeof(eg3d_similarity_stats)) return EG3D_TRANSFORM_ERR_ARG;
  int used = 0;
  for (int i = 0; i < n; i++)
    if (!(null_mask && null_mask[i])) {
      if (!finite3(src + 3 * i) || !finite3(dst + 3 * i)) return EG3D_TRANSFORM_ERR_NONFINITE;
      used++;
    }
  if (used < 3) return EG3D_TRANSFORM_ERR_FEW;
  const double one_over_n = 1.0 / (double)used;
  double ms[3] = {0, 0, 0}, md[3] = {0, 0, 0};
  for (int i = 0; i < n; i++)
    if (!(null_mask && null_mask[i]))
      for (int k = 0; k < 3; k++) {
        ms[k] += src[3 * i + k];
        md[k] += dst[3 * i + k];
      }
  for (int k = 0; k < 3; k++) {
    ms[k] *= one_over_n;
    md[k] *= one_over_n;
  }
  double var = 0, raw = 0, sigma[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int i = 0; i < n; i++)
    if (!(null_mask && null_mask[i])) {
      double a[3], b[3];
      for (int k = 0; k < 3; k++) {
        a[k] = src[3 * i + k] - ms[k];
        b[k] = dst[3 * i + k] - md[k];
      }
      raw += (src[3 * i] * src[3 * i] + src[3 * i + 1] * src[3 * i + 1]) + src[3 * i + 2] * src[3 * i + 2];
      var += (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) sigma[r][c] += b[r] * a[c];
    }
  var *= one_over_n;
  if (!std::isfinite(var)) return EG3D_TRANSFORM_ERR_NONFINITE;  // (finite centres whose squares overflow)
  // all source centres equal: src_var is 0, or what the rounding of the mean leaves of it (a spread below 1e-14 of the
  // centres' own magnitude)
  if (var == 0.0 || var <= kDegenerate * (raw * one_over_n)) return EG3D_TRANSFORM_ERR_DEGENERATE;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) sigma[r][c] *= one_over_n;
  double U[3][3], V[3][3], d[3];
  const int rank = svd3(sigma, U, d, V);
  const bool reflect = det3(U) * det3(V) < 0.0;
  const double S[3] = {1.0, 1.0, reflect ? -1.0 : 1.0};
  double R[3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[r][c] = (U[r][0] * S[0] * V[c][0] + U[r][1] * S[1] * V[c][1]) + U[r][2] * S[2] * V[c][2];
  const double scale = ((d[0] * S[0] + d[1] * S[1]) + d[2] * S[2]) / var;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[4 * r + c] = scale * R[r][c];
    T[4 * r + 3] = md[r] - ((scale * R[r][0] * ms[0] + scale * R[r][1] * ms[1]) + scale * R[r][2] * ms[2]);
  }
  T[12] = T[13] = T[14] = 0.0;
  T[15] = 1.0;
  if (stats) {
    stats->struct_size = (uint32_t)sizeof(eg3d_similarity_stats);
    stats->n_used = (uint32_t)used;
    stats->scale = scale;
    for (int k = 0; k < 3; k++) stats->singular[k] = d[k];
    stats->src_var = var;
    stats->reflection = reflect ? 1u : 0u;
    stats->rank_deficient = rank < 2 ? 1u : 0u;
  }
  return EG3D_TRANSFORM_OK;
}

extern "C" int eg3d_host_transform_points(const double* T, const float* X, uint64_t n, float* X_out) {
  if (!T || (n && (!X || !X_out))) return EG3D_TRANSFORM_ERR_ARG;
  const Mat4 M = to_f32(T);
#pragma omp parallel for schedule(static) if (n >= (1u << 16))
  for (long long i = 0; i < (long long)n; i++) point(M, X + 3 * i, X_out + 3 * i);  // (a point is read whole before it is written)
  return EG3D_TRANSFORM_OK;
}

extern "C" int eg3d_host_transform_cameras(const double* T, int n, const float* fpp, float* R9, float* C3, float* t3, float* P16) {
  if (!T || n < 0 || (n && (!fpp || !R9 || !C3 || !t3 || !P16))) return EG3D_TRANSFORM_ERR_ARG;
  for (int k = 0; k < 16; k++)
    if (!std::isfinite(T[k])) return EG3D_TRANSFORM_ERR_NONFINITE;
  const Mat4 M = to_f32(T);
  const Mat4 I = inverse(M);
  for (int v = 0; v < n; v++) {
    float *R = R9 + 9 * v, *C = C3 + 3 * v, *t = t3 + 3 * v, *P = P16 + 16 * v;
    if (is_null(R, C)) continue;
    Mat4 E, K;
    memset(&E, 0, sizeof(E));
    memset(&K, 0, sizeof(K));
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) E.m[r][c] = R[3 * r + c];
      E.m[r][3] = t[r];
    }
    E.m[3][3] = 1.0f;
    K.m[0][0] = fpp[3 * v];
    K.m[1][1] = fpp[3 * v];
    K.m[0][2] = fpp[3 * v + 1];
    K.m[1][2] = fpp[3 * v + 2];
    K.m[2][2] = 1.0f;
    const Mat4 e = mul(I, E);
    const Mat4 p = mul(e, K);
    memcpy(P, p.m, sizeof(float) * 16);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) R[3 * r + c] = e.m[r][c];
      t[r] = e.m[r][3];
    }
    float Cn[3];
    point(M, C, Cn);
    memcpy(C, Cn, sizeof(Cn));
  }
  return EG3D_TRANSFORM_OK;
}

extern "C" int eg3d_host_glm_inverse4(const float* m16, float* out16) {
  if (!m16 || !out16) return EG3D_TRANSFORM_ERR_ARG;
  Mat4 a;
  memcpy(a.m, m16, sizeof(a.m));
  const Mat4 r = inverse(a);
  memcpy(out16, r.m, sizeof(r.m));
  return EG3D_TRANSFORM_OK;
}
extern "C" int eg3d_host_glm_mul4(const float* a16, const float* b16, float* out16) {
  if (!a16 || !b16 || !out16) return EG3D_TRANSFORM_ERR_ARG;
  Mat4 a, b;
  memcpy(a.m, a16, sizeof(a.m));
  memcpy(b.m, b16, sizeof(b.m));
  const Mat4 r = mul(a, b);
  memcpy(out16, r.m, sizeof(r.m));
  return EG3D_TRANSFORM_OK;
}

extern "C" int eg3d_host_camera_errors(int n, const float* C3, const uint8_t* null_mask, const double* target, float* out) {
  if (n < 0 || !out || (n && (!C3 || !target))) return EG3D_TRANSFORM_ERR_ARG;
  float sum = 0;
  for (int i = 0; i < n; i++) {
    if (null_mask && null_mask[i]) continue;
    const double dx = (double)C3[3 * i] - target[3 * i], dy = (double)C3[3 * i + 1] - target[3 * i + 1],
                 dz = (double)C3[3 * i + 2] - target[3 * i + 2];
    sum = (float)((double)sum + std::sqrt((dx * dx + dy * dy) + dz * dz));
  }
  *out = sum / (float)n;  // Q16: ALL cameras, null ones included
  return EG3D_TRANSFORM_OK;
}
