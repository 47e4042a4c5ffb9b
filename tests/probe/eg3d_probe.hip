// TEST-ONLY library (tests/probe/libeg3d_probe.so, built by edgegraph3d_amd.build.build_probe): runs
// single device primitives of the product's headers (IEEE arithmetic, DLT, triangulation) on the
// GPU so that tests/test_gpu_arith.py can check the arithmetic contract bit-for-bit against x86 and
// the oracle. Nothing of this is linked into libeg3d.so.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "eg3d_probe.h"
#include "eg3d_dev_pipeline.h"
#include "eg3d_dev_coopgn.h"
#include "eg3d_geom_items.h"

using namespace eg3d;

__global__ void k_probe_arith(uint64_t n, const double* a, const double* b, const double* c, double* od, const float* fa,
                              const float* fb, const float* fc, float* of) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  od[0 * n + i] = a[i] / b[i];
  od[1 * n + i] = EG3D_SQRT(absd(a[i]));
  double p = a[i] * b[i];
  od[2 * n + i] = p + c[i];
  od[3 * n + i] = (double)(float)a[i];
  od[4 * n + i] = 1. / EG3D_SQRT(absd(b[i]));
  of[0 * n + i] = fa[i] / fb[i];
  of[1 * n + i] = EG3D_SQRTF(EG3D_FABSF(fa[i]));
  float q = fa[i] * fb[i];
  of[2 * n + i] = q + fc[i];
  of[3 * n + i] = dist2(fa[i], fb[i], fc[i], fa[i]);
  of[4 * n + i] = __builtin_sqrtf(EG3D_FABSF(fa[i]));
}

__global__ void k_probe_tri(const float* cam_P, uint64_t n, int k, const int32_t* views, const float* xy, float* X,
                            uint8_t* valid, double* dlt) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Obs a[16];
  for (int j = 0; j < k && j < 16; j++) {
    a[j].view = views[i * k + j];
    a[j].pl = 0;
    a[j].seg = 0;
    a[j].x = xy[2 * (i * k + j)];
    a[j].y = xy[2 * (i * k + j) + 1];
  }
  uint32_t flags = 0;
  float Xo[3] = {0, 0, 0};
  bool ok = triangulate_array(cam_P, a, k, Xo, flags);
  valid[i] = ok;
  X[3 * i] = Xo[0];
  X[3 * i + 1] = Xo[1];
  X[3 * i + 2] = Xo[2];
  int mi = 0;
  for (int j = 0; j < k; j++)
    if (a[j].view < a[mi].view) mi = j;
  double X0[3];
  dlt2(cam_P + (size_t)a[mi].view * 16, a[mi].x, a[mi].y, cam_P + (size_t)a[k - 1].view * 16, a[k - 1].x, a[k - 1].y, X0);
  dlt[3 * i] = X0[0];
  dlt[3 * i + 1] = X0[1];
  dlt[3 * i + 2] = X0[2];
}

// the 2-view DLT on groups of 8 lanes (dlt2_grp8): item i on group (i % 8) of block (i / 8); same operand choice as
// k_probe_tri (minimum view id, last observation)
__global__ void __launch_bounds__(64) k_probe_dlt_grp(const float* cam_P, uint64_t n, int k, const int32_t* views, const float* xy,
                                                      double* dlt) {
  __shared__ DltGrpLds S;
  const int lane = (int)threadIdx.x, g = lane >> 3;
  const uint64_t i = (uint64_t)blockIdx.x * 8 + (uint64_t)g;
  const bool on = i < n;
  const float* P1 = cam_P;
  const float* P2 = cam_P;
  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
  if (on) {
    int mi = 0;
    for (int j = 0; j < k; j++)
      if (views[i * k + j] < views[i * k + mi]) mi = j;
    P1 = cam_P + (size_t)views[i * k + mi] * 16;
    x1 = xy[2 * (i * k + mi)];
    y1 = xy[2 * (i * k + mi) + 1];
    P2 = cam_P + (size_t)views[i * k + k - 1] * 16;
    x2 = xy[2 * (i * k + k - 1)];
    y2 = xy[2 * (i * k + k - 1) + 1];
  }
  double X0[3] = {0, 0, 0};
  dlt2_grp8(S, on, P1, x1, y1, P2, x2, y2, X0);
  if (on && (lane & 7) == 0) {
    dlt[3 * i] = X0[0];
    dlt[3 * i + 1] = X0[1];
    dlt[3 * i + 2] = X0[2];
  }
}

#define PT(expr)                         \
  do {                                   \
    if ((expr) != hipSuccess) return -2; \
  } while (0)

extern "C" int eg3d_probe_dlt_rows(void) { return EG3D_DLT_ROWS; }

extern "C" int eg3d_probe_arith(uint64_t n, const double* a, const double* b, const double* c, double* od,
                                const float* fa, const float* fb, const float* fc, float* of) {
  double *da, *db, *dc, *dod;
  float *dfa, *dfb, *dfc, *dof;
  PT(hipMalloc(&da, n * 8));
  PT(hipMalloc(&db, n * 8));
  PT(hipMalloc(&dc, n * 8));
  PT(hipMalloc(&dod, n * 8 * 5));
  PT(hipMalloc(&dfa, n * 4));
  PT(hipMalloc(&dfb, n * 4));
  PT(hipMalloc(&dfc, n * 4));
  PT(hipMalloc(&dof, n * 4 * 5));
  PT(hipMemcpy(da, a, n * 8, hipMemcpyHostToDevice));
  PT(hipMemcpy(db, b, n * 8, hipMemcpyHostToDevice));
  PT(hipMemcpy(dc, c, n * 8, hipMemcpyHostToDevice));
  PT(hipMemcpy(dfa, fa, n * 4, hipMemcpyHostToDevice));
  PT(hipMemcpy(dfb, fb, n * 4, hipMemcpyHostToDevice));
  PT(hipMemcpy(dfc, fc, n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe_arith, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, da, db, dc, dod, dfa, dfb, dfc,
                     dof);
  PT(hipDeviceSynchronize());
  PT(hipMemcpy(od, dod, n * 8 * 5, hipMemcpyDeviceToHost));
  PT(hipMemcpy(of, dof, n * 4 * 5, hipMemcpyDeviceToHost));
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dc);
  (void)hipFree(dod);
  (void)hipFree(dfa);
  (void)hipFree(dfb);
  (void)hipFree(dfc);
  (void)hipFree(dof);
  return 0;
}

extern "C" int eg3d_probe_triangulate(const float* cam_P, int n_views, uint64_t n, int k, const int32_t* views,
                                      const float* xy, float* X, uint8_t* valid, double* dlt) {
  if (!cam_P || n_views < 1 || k < 2 || k > 16) return -1;
  int32_t* dv;
  float *dxy, *dX, *dP;
  PT(hipMalloc(&dP, (size_t)n_views * 64));
  PT(hipMemcpy(dP, cam_P, (size_t)n_views * 64, hipMemcpyHostToDevice));
  uint8_t* dval;
  double* ddlt;
  PT(hipMalloc(&dv, n * k * 4));
  PT(hipMalloc(&dxy, n * k * 8));
  PT(hipMalloc(&dX, n * 12));
  PT(hipMalloc(&dval, n));
  PT(hipMalloc(&ddlt, n * 24));
  PT(hipMemcpy(dv, views, n * k * 4, hipMemcpyHostToDevice));
  PT(hipMemcpy(dxy, xy, n * k * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe_tri, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, dP, n, k, dv, dxy, dX, dval, ddlt);
  PT(hipDeviceSynchronize());
  PT(hipMemcpy(X, dX, n * 12, hipMemcpyDeviceToHost));
  PT(hipMemcpy(valid, dval, n, hipMemcpyDeviceToHost));
  PT(hipMemcpy(dlt, ddlt, n * 24, hipMemcpyDeviceToHost));
  (void)hipFree(dP);
  (void)hipFree(dv);
  (void)hipFree(dxy);
  (void)hipFree(dX);
  (void)hipFree(dval);
  (void)hipFree(ddlt);
  return 0;
}

extern "C" int eg3d_probe_dlt_groups(const float* cam_P, int n_views, uint64_t n, int k, const int32_t* views, const float* xy,
                                     double* dlt) {
  if (!cam_P || n_views < 1 || k < 2 || k > 16 || !n) return -1;
  int32_t* dv;
  float *dxy, *dP;
  double* ddlt;
  PT(hipMalloc(&dP, (size_t)n_views * 64));
  PT(hipMemcpy(dP, cam_P, (size_t)n_views * 64, hipMemcpyHostToDevice));
  PT(hipMalloc(&dv, n * k * 4));
  PT(hipMalloc(&dxy, n * k * 8));
  PT(hipMalloc(&ddlt, n * 24));
  PT(hipMemcpy(dv, views, n * k * 4, hipMemcpyHostToDevice));
  PT(hipMemcpy(dxy, xy, n * k * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe_dlt_grp, dim3((unsigned)((n + 7) / 8)), dim3(64), 0, 0, dP, n, k, dv, dxy, ddlt);
  PT(hipDeviceSynchronize());
  PT(hipMemcpy(dlt, ddlt, n * 24, hipMemcpyDeviceToHost));
  (void)hipFree(dP);
  (void)hipFree(dv);
  (void)hipFree(dxy);
  (void)hipFree(ddlt);
  return 0;
}

// ---- the shared-reciprocal divisions of the Gauss-Newton rows (eg3d_dev_coopgn.h) against plain divisions ----
// pairs: out[0][i] = num / den (the compiler's full sequence), out[1][i] = gn_div(num, gn_recip(den)),
// out[2][i] = 1 when den is in the range the row test admits. rows: GnRow of the plain and of the guarded fast path.
__global__ void k_probe_gn_div(uint64_t n, const double* num, const double* den, double* out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = num[i] / den[i];
  const GnRecip R = gn_recip(den[i]);
  out[n + i] = gn_div(num[i], R);
  out[2 * n + i] = gn_mid_range(den[i]) ? 1.0 : 0.0;
}
__global__ void k_probe_gn_rows(uint64_t n, const float* P, const float* oxy, const double* X, double* out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double Xi[3] = {X[3 * i], X[3 * i + 1], X[3 * i + 2]};
  GnRow a, b;
  gn_row(P + 16 * i, oxy[2 * i], oxy[2 * i + 1], Xi, a, false);
  gn_row(P + 16 * i, oxy[2 * i], oxy[2 * i + 1], Xi, b, true);
  const double va[8] = {a.j00, a.j01, a.j02, a.j10, a.j11, a.j12, a.r0, a.r1};
  const double vb[8] = {b.j00, b.j01, b.j02, b.j10, b.j11, b.j12, b.r0, b.r1};
  for (int k = 0; k < 8; k++) {
    out[(size_t)k * n + i] = va[k];
    out[(size_t)(8 + k) * n + i] = vb[k];
  }
}
extern "C" int eg3d_probe_gn_div(uint64_t n, const double* num, const double* den, double* out3n) {
  double *dn, *dd, *dout;
  PT(hipMalloc(&dn, n * 8));
  PT(hipMalloc(&dd, n * 8));
  PT(hipMalloc(&dout, n * 8 * 3));
  PT(hipMemcpy(dn, num, n * 8, hipMemcpyHostToDevice));
  PT(hipMemcpy(dd, den, n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe_gn_div, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, dn, dd, dout);
  PT(hipDeviceSynchronize());
  PT(hipMemcpy(out3n, dout, n * 8 * 3, hipMemcpyDeviceToHost));
  (void)hipFree(dn);
  (void)hipFree(dd);
  (void)hipFree(dout);
  return 0;
}
extern "C" int eg3d_probe_gn_rows(uint64_t n, const float* P16, const float* oxy, const double* X, double* out16n) {
  float *dP, *dxy;
  double *dX, *dout;
  PT(hipMalloc(&dP, n * 64));
  PT(hipMalloc(&dxy, n * 8));
  PT(hipMalloc(&dX, n * 24));
  PT(hipMalloc(&dout, n * 8 * 16));
  PT(hipMemcpy(dP, P16, n * 64, hipMemcpyHostToDevice));
  PT(hipMemcpy(dxy, oxy, n * 8, hipMemcpyHostToDevice));
  PT(hipMemcpy(dX, X, n * 24, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe_gn_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, dP, dxy, dX, dout);
  PT(hipDeviceSynchronize());
  PT(hipMemcpy(out16n, dout, n * 8 * 16, hipMemcpyDeviceToHost));
  (void)hipFree(dP);
  (void)hipFree(dxy);
  (void)hipFree(dX);
  (void)hipFree(dout);
  return 0;
}

// ---- the lane-group Gauss-Newton solver AT FULL DENSITY (tools/gn_floor.py): every single-wave block solves `rounds` windows
// of SEVEN identical ADD requests of n rows each (7 x 9 = 63 of the 64 rows of a packed round; identical requests converge in
// the same iteration, so no lane waits for another request) through coop_gn_groups — the product's solver, the product's
// build switches, 4 waves per SIMD like the expand kernel. What comes out is the solver's speed of light on this chip under
// the arithmetic contract (FP64, no FMA, ordered sums): row-iterations per second.
__global__ void __launch_bounds__(64, 4) k_probe_gn_dense(const float* cam_P, const Obs* obs, int n, float x0, float y0, float z0,
                                                          int rounds, float* out) {
  __shared__ CoopLds L;
  const int lane = (int)threadIdx.x;
  if (lane == 0) {
    L.cams_mid_range = 1;
    L.long_refused = 0;
  }
  __syncthreads();
  float acc = 0.0f;
  int n_ok = 0;
  for (int r = 0; r < rounds; r++) {
    const float X0[3] = {x0, y0, z0};
    float X[3] = {0.0f, 0.0f, 0.0f};
    const Obs ex = obs[n - 1];
    const bool ok = coop_gn_groups<0, false>(cam_P, L, lane < 7, obs, n - 1, true, (int32_t)ex.view, ex.x, ex.y, X0, X);
    acc += X[0];
    n_ok += ok ? 1 : 0;
  }
  if (lane == 0) {
    out[4 * blockIdx.x] = acc / (float)rounds;
    out[4 * blockIdx.x + 1] = (float)n_ok;
  }
}
// obs_view / obs_xy: the n observations of the request (the last one is the ADD observation); returns the kernel time in ms
// and, in X_ok[0..1], block 0's mean solution x and the number of accepted solves of its lane 0
extern "C" int eg3d_probe_gn_dense(const float* cam_P, int n_views, const int32_t* obs_view, const float* obs_xy, int n,
                                   const float* X0, int n_blocks, int rounds, float* ms, float* X_ok) {
  if (n < 3 || n > 9 || n_blocks < 1 || rounds < 1) return -1;
  float* dP;
  Obs* dobs;
  float* dout;
  std::vector<Obs> h((size_t)n);
  for (int i = 0; i < n; i++) {
    h[i].view = (uint32_t)obs_view[i];
    h[i].pl = 0;
    h[i].seg = 0;
    h[i].x = obs_xy[2 * i];
    h[i].y = obs_xy[2 * i + 1];
  }
  PT(hipMalloc(&dP, (size_t)n_views * 64));
  PT(hipMalloc(&dobs, sizeof(Obs) * (size_t)n));
  PT(hipMalloc(&dout, sizeof(float) * 4 * (size_t)n_blocks));
  PT(hipMemcpy(dP, cam_P, (size_t)n_views * 64, hipMemcpyHostToDevice));
  PT(hipMemcpy(dobs, h.data(), sizeof(Obs) * (size_t)n, hipMemcpyHostToDevice));
  hipEvent_t a, b;
  PT(hipEventCreate(&a));
  PT(hipEventCreate(&b));
  hipLaunchKernelGGL(k_probe_gn_dense, dim3((unsigned)n_blocks), dim3(64), 0, 0, dP, dobs, n, X0[0], X0[1], X0[2], 2, dout);  // warm-up
  PT(hipEventRecord(a, 0));
  hipLaunchKernelGGL(k_probe_gn_dense, dim3((unsigned)n_blocks), dim3(64), 0, 0, dP, dobs, n, X0[0], X0[1], X0[2], rounds, dout);
  PT(hipEventRecord(b, 0));
  PT(hipDeviceSynchronize());
  PT(hipEventElapsedTime(ms, a, b));
  float r[4];
  PT(hipMemcpy(r, dout, sizeof(r), hipMemcpyDeviceToHost));
  X_ok[0] = r[0];
  X_ok[1] = r[1];
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  (void)hipFree(dP);
  (void)hipFree(dobs);
  (void)hipFree(dout);
  return 0;
}

// ---- the lane-group Gauss-Newton solver, request by request (tests/test_gpu_coop_gn.py): one single-wave block per window of
// up to EG3D_COOP_REQ requests (request j on lane j, lanes without one pass want = false), coop_gn_groups called exactly as
// k3b_expand calls it, with the template arguments of the product's instantiations (TeamWaveT, eg3d_k3b_expand.h) taken from
// the same macros. Verdict and solution of every request, and the window's long_refused, go back to the host.
template <int KEEP, bool LONG_GN, int PRE_IT>
__global__ void __launch_bounds__(64) k_probe_coop_gn(const float* cam_P, const Obs* obs, const int32_t* req_i, const float* req_f,
                                                      int cams_mid_range, uint8_t* valid, float* Xo, uint8_t* refused) {
  __shared__ CoopLds L;
  const int lane = (int)threadIdx.x;
  const size_t e = (size_t)blockIdx.x * EG3D_COOP_REQ + (size_t)lane;
  if (lane == 0) {
    L.cams_mid_range = cams_mid_range ? 1 : 0;
    L.long_refused = 0;
  }
  __syncthreads();
  bool want = false, has_extra = false;
  const Obs* base = obs;
  int nblock = 0;
  int32_t ex_view = 0;
  float ex_x = 0.f, ex_y = 0.f;
  float X0[3] = {0.f, 0.f, 0.f};
  if (lane < EG3D_COOP_REQ) {
    const int32_t* q = req_i + 5 * e;
    const float* f = req_f + 5 * e;
    want = q[0] != 0;
    if (want) {
      base = obs + q[1];
      nblock = q[2];
      has_extra = q[3] != 0;
      ex_view = q[4];
      ex_x = f[0];
      ex_y = f[1];
    }
    X0[0] = f[2];
    X0[1] = f[3];
    X0[2] = f[4];
  }
  float X[3] = {0.f, 0.f, 0.f};
  const bool ok = coop_gn_groups<KEEP, LONG_GN, PRE_IT>(cam_P, L, want, base, nblock, has_extra, ex_view, ex_x, ex_y, X0, X);
  if (lane < EG3D_COOP_REQ) {
    valid[e] = ok ? 1 : 0;
    Xo[3 * e] = X[0];
    Xo[3 * e + 1] = X[1];
    Xo[3 * e + 2] = X[2];
  }
  __syncthreads();
  if (lane == 0) refused[blockIdx.x] = L.long_refused;
}

// The group size coop_gn_run gives each request of a window, its rules restated: a short request (<= EG3D_GN_PACK_MAX rows) is
// one group of its own row count; the long ones go in lane order, round after round, the first 64 >> lg of those left
// getting groups of 2^lg lanes, lg chosen by the cost model over the longest request left. 0 = not solved.
static void coop_gn_group_sizes(int keep, bool long_gn, const int* n_req, int32_t* G) {
  std::vector<int> todo;
  for (int j = 0; j < EG3D_COOP_REQ; j++) {
    G[j] = 0;
    if (n_req[j] > 0 && n_req[j] <= EG3D_GN_PACK_MAX) G[j] = n_req[j];
    if (n_req[j] > EG3D_GN_PACK_MAX) todo.push_back(j);
  }
  if (!long_gn) return;
  while (!todo.empty()) {
    const int Bl = (int)todo.size();
    int mxl = 0;
    for (int j : todo) mxl = n_req[j] > mxl ? n_req[j] : mxl;
    int lg = 6;
    unsigned best = 0xffffffffu;
    for (int cand = 1; cand <= 6; cand++) {
      const int Gc = 1 << cand;
      const int k = (mxl + Gc - 1) >> cand;
      const int rounds = (Bl + (64 >> cand) - 1) / (64 >> cand);
      const int krow = keep == 0 ? (k > 1 ? 2 * k : k) : k + (k > keep ? k - keep : 0);
      const unsigned cost = (unsigned)rounds * ((unsigned)krow * EG3D_GN_ROW_CYCLES + (unsigned)k * EG3D_GN_SUM_CYCLES * Gc);
      if (cost < best) {
        best = cost;
        lg = cand;
      }
    }
    const int per_round = 64 >> lg;
    const int take = Bl < per_round ? Bl : per_round;
    for (int t = 0; t < take; t++) G[todo[t]] = 1 << lg;
    todo.erase(todo.begin(), todo.begin() + take);
  }
}

extern "C" int eg3d_probe_coop_gn_variants(void) { return 6; }

extern "C" int eg3d_probe_coop_gn(int variant, const float* cam_P, int n_views, const int32_t* obs_view, const float* obs_xy,
                                  uint64_t n_obs, int n_windows, const int32_t* req_i, const float* req_f, int cams_mid_range,
                                  uint8_t* valid, float* X, int32_t* G, uint8_t* long_refused) {
  static const int keep_of[6] = {0, 0, EG3D_MANY_KEEP, 2, 0, 0};
  static const bool long_of[6] = {false, true, true, true, true, false};
  if (variant < 0 || variant > 5 || !cam_P || n_views < 1 || n_views >= (1 << EG3D_VIEW_BITS) || !obs_view || !obs_xy ||
      n_obs < 1 || n_obs > 0x7fffffffull || n_windows < 1)
    return -1;
  for (uint64_t i = 0; i < n_obs; i++)
    if (obs_view[i] < 0 || obs_view[i] >= n_views) return -1;
  const size_t ne = (size_t)n_windows * EG3D_COOP_REQ;
  std::vector<int> n_req(ne, 0);
  for (size_t e = 0; e < ne; e++) {
    const int32_t* q = req_i + 5 * e;
    if (!q[0]) continue;
    if (q[1] < 0 || q[2] < 0 || (uint64_t)q[1] + (uint64_t)q[2] > n_obs) return -1;
    if (q[3] && (q[4] < 0 || q[4] >= n_views)) return -1;
    n_req[e] = q[2] + (q[3] ? 1 : 0);
    if (n_req[e] < 2 || n_req[e] > 0x7fff) return -1;  // every request >= 2 rows; n16 holds 15 bits of row count
  }
  for (int w = 0; w < n_windows; w++)
    coop_gn_group_sizes(keep_of[variant], long_of[variant], &n_req[(size_t)w * EG3D_COOP_REQ], G + (size_t)w * EG3D_COOP_REQ);
  std::vector<Obs> h((size_t)n_obs);
  for (uint64_t i = 0; i < n_obs; i++) {
    h[i].view = (uint32_t)obs_view[i];
    h[i].pl = 0;
    h[i].seg = 0;
    h[i].x = obs_xy[2 * i];
    h[i].y = obs_xy[2 * i + 1];
  }
  float *dP, *df, *dX;
  Obs* dobs;
  int32_t* di;
  uint8_t *dval, *dref;
  PT(hipMalloc(&dP, (size_t)n_views * 64));
  PT(hipMalloc(&dobs, sizeof(Obs) * (size_t)n_obs));
  PT(hipMalloc(&di, ne * 5 * 4));
  PT(hipMalloc(&df, ne * 5 * 4));
  PT(hipMalloc(&dval, ne));
  PT(hipMalloc(&dX, ne * 12));
  PT(hipMalloc(&dref, (size_t)n_windows));
  PT(hipMemcpy(dP, cam_P, (size_t)n_views * 64, hipMemcpyHostToDevice));
  PT(hipMemcpy(dobs, h.data(), sizeof(Obs) * (size_t)n_obs, hipMemcpyHostToDevice));
  PT(hipMemcpy(di, req_i, ne * 5 * 4, hipMemcpyHostToDevice));
  PT(hipMemcpy(df, req_f, ne * 5 * 4, hipMemcpyHostToDevice));
  const dim3 grid((unsigned)n_windows), block(64);
  switch (variant) {
    case 0:  // small scenes (TeamWaveT<0, 0>)
      hipLaunchKernelGGL((k_probe_coop_gn<0, false, 30>), grid, block, 0, 0, dP, dobs, di, df, cams_mid_range, dval, dX, dref);
      break;
    case 1:  // general (TeamWaveT<0, 1>)
      hipLaunchKernelGGL((k_probe_coop_gn<0, true, 30>), grid, block, 0, 0, dP, dobs, di, df, cams_mid_range, dval, dX, dref);
      break;
    case 2:  // many views (TeamWaveT<EG3D_MANY_KEEP, 2>)
      hipLaunchKernelGGL((k_probe_coop_gn<EG3D_MANY_KEEP, true, EG3D_GN_PRECHECK_IT>), grid, block, 0, 0, dP, dobs, di, df,
                         cams_mid_range, dval, dX, dref);
      break;
    case 3:  // the many-views build with two kept chunks (EG3D_MANY_KEEP=2)
      hipLaunchKernelGGL((k_probe_coop_gn<2, true, EG3D_GN_PRECHECK_IT>), grid, block, 0, 0, dP, dobs, di, df, cams_mid_range,
                         dval, dX, dref);
      break;
    case 4:  // the general build with the pre-check (EG3D_GN_PRECHECK_ALL=1)
      hipLaunchKernelGGL((k_probe_coop_gn<0, true, EG3D_GN_PRECHECK_IT>), grid, block, 0, 0, dP, dobs, di, df, cams_mid_range,
                         dval, dX, dref);
      break;
    default:  // the small build with the pre-check (EG3D_GN_PRECHECK_ALL=1)
      hipLaunchKernelGGL((k_probe_coop_gn<0, false, EG3D_GN_PRECHECK_IT>), grid, block, 0, 0, dP, dobs, di, df, cams_mid_range,
                         dval, dX, dref);
      break;
  }
  PT(hipGetLastError());
  PT(hipDeviceSynchronize());
  PT(hipMemcpy(valid, dval, ne, hipMemcpyDeviceToHost));
  PT(hipMemcpy(X, dX, ne * 12, hipMemcpyDeviceToHost));
  PT(hipMemcpy(long_refused, dref, (size_t)n_windows, hipMemcpyDeviceToHost));
  (void)hipFree(dP);
  (void)hipFree(dobs);
  (void)hipFree(di);
  (void)hipFree(df);
  (void)hipFree(dval);
  (void)hipFree(dX);
  (void)hipFree(dref);
  return 0;
}

// ---- the 2-D geometry primitives the glm pin test checks (tests/test_glm_pin.py): project_f32, seg_line_cos,
// seg_closest of the product's headers on the GPU. in = [n][19] / [n][7] / [n][6] floats as tests/glm/glm_driver.cpp takes.
__global__ void k_probe_geom(uint64_t n, int mode, const float* in, float* out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (mode == 0) {
    const float* q = in + 19 * i;
    float u, v;
    project_f32(q, q[16], q[17], q[18], u, v);
    out[2 * i] = u;
    out[2 * i + 1] = v;
  } else if (mode == 1) {
    const float* q = in + 7 * i;
    out[i] = seg_line_cos(q[0], q[1], q[2], q[3], q[4], q[5]);
  } else {
    const float* q = in + 6 * i;
    float qx, qy;
    out[3 * i] = seg_closest(q[0], q[1], q[2], q[3], q[4], q[5], qx, qy);
    out[3 * i + 1] = qx;
    out[3 * i + 2] = qy;
  }
}
extern "C" int eg3d_probe_geom(uint64_t n, int mode, const float* in, float* out) {
  const size_t rin = mode == 0 ? 19 : mode == 1 ? 7 : 6, rout = mode == 0 ? 2 : mode == 1 ? 1 : 3;
  float *di, *dout;
  PT(hipMalloc(&di, n * rin * 4));
  PT(hipMalloc(&dout, n * rout * 4));
  PT(hipMemcpy(di, in, n * rin * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe_geom, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, mode, di, dout);
  PT(hipDeviceSynchronize());
  PT(hipMemcpy(out, dout, n * rout * 4, hipMemcpyDeviceToHost));
  (void)hipFree(di);
  (void)hipFree(dout);
  return 0;
}

// ---- the geometry and walk primitives of eg3d_dev_geom.h (and epiline) ITEM BY ITEM (tests/test_gpu_geom_primitives.py): one
// row of a table of tests/geom_cases.py per lane, one primitive call per row (eg3d_geom_items.h: the same items the host
// simulation runs through the host compilation of the header). Every loop on the device is one of the header's own, bounded by
// the polyline's length; the host side refuses a table that breaks the input contract (-1) before anything is launched, and
// every vertex array carries one spare vertex behind its last one.
namespace gi = eg3d_items;

// the launch's own error goes back as its (positive) HIP code
#define PT_LAUNCH()                        \
  do {                                     \
    const hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) return (int)e_;  \
  } while (0)

// device memory that frees itself, so that a refused table or a failed copy leaks nothing
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
  hipError_t up(const void* src, size_t bytes) {
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess || !bytes) return e;
    return hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
  }
  hipError_t down(void* dst, size_t bytes) const { return bytes ? hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
};

struct WalkTab {
  const f2* vtx;
  const uint32_t *pl_off, *pl_start, *pl_end;
  const uint32_t *row_pl, *row_seg, *row_dir;
  const float* row_f;
  const uint8_t* row_bnd;
  uint32_t *status, *seg;
  float* xy;
};

__global__ void __launch_bounds__(256) k_probe_walk(int form, uint64_t n, WalkTab t) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = t.row_pl[i];
  PlRef pl;
  pl.v = t.vtx + t.pl_off[p];
  pl.n = t.pl_off[p + 1] - t.pl_off[p];
  pl.start = t.pl_start[p];
  pl.end = t.pl_end[p];
  PlPt o;
  o.seg = t.seg[i];
  o.x = t.xy[2 * i];
  o.y = t.xy[2 * i + 1];
  t.status[i] = gi::walk_item(form, pl, t.row_seg[i], t.row_dir[i], t.row_f + 8 * i, t.row_bnd[i] != 0, o);
  t.seg[i] = o.seg;
  t.xy[2 * i] = o.x;
  t.xy[2 * i + 1] = o.y;
}

// walk_by_line on an address_space(3) pointer, as the expand kernel's side walks instantiate it (PlRefT<lds_f2p>,
// eg3d_k3b_expand.h): block b stages the polyline blk[b][0] in LDS and its lanes take the rows blk[b][1] .. blk[b][2] - 1
// (at most one per lane), all of that polyline. A polyline of more than EG3D_PROBE_LDS_VTX vertices gets no block.
#define EG3D_PROBE_LDS_VTX 512
__global__ void __launch_bounds__(256) k_probe_walk_lds(const uint32_t* blk, WalkTab t) {
  typedef const __attribute__((address_space(3))) f2* lds_f2p;
  __shared__ f2 sv[EG3D_PROBE_LDS_VTX + 1];
  const uint32_t p = blk[3 * blockIdx.x];
  const uint32_t v0 = t.pl_off[p], nvert = t.pl_off[p + 1] - v0;
  for (uint32_t k = threadIdx.x; k < nvert + 1 && k < EG3D_PROBE_LDS_VTX + 1; k += blockDim.x) sv[k] = t.vtx[v0 + k];  // + the spare one
  __syncthreads();
  const uint64_t i = (uint64_t)blk[3 * blockIdx.x + 1] + threadIdx.x;
  if (i >= blk[3 * blockIdx.x + 2]) return;
  PlRefT<lds_f2p> pl;
  pl.v = (lds_f2p)&sv[0];
  pl.n = nvert;
  pl.start = t.pl_start[p];
  pl.end = t.pl_end[p];
  const float* f = t.row_f + 8 * i;
  PlPt q, o;
  q.seg = t.row_seg[i];
  q.x = f[0];
  q.y = f[1];
  o.seg = t.seg[i];
  o.x = t.xy[2 * i];
  o.y = t.xy[2 * i + 1];
  t.status[i] = walk_by_line(pl, q, t.row_dir[i], f[2], f[3], f[4], t.row_bnd[i] != 0, f[6], f[7], o);
  t.seg[i] = o.seg;
  t.xy[2 * i] = o.x;
  t.xy[2 * i + 1] = o.y;
}

extern "C" int eg3d_probe_walk_lds_capacity(void) { return EG3D_PROBE_LDS_VTX; }

extern "C" int eg3d_probe_walk(int form, const float* vtx, uint64_t nv, const uint32_t* pl_off, const uint32_t* pl_start,
                               const uint32_t* pl_end, uint32_t npl, uint64_t n, const uint32_t* row_pl, const uint32_t* row_seg,
                               const uint32_t* row_dir, const float* row_f, const uint8_t* row_bnd, uint32_t* status, uint32_t* seg,
                               float* xy) {
  if (form < 0 || form >= gi::WALK_N_FORMS || !n || n > 0x7fffffffull || nv > 0x7fffffffull) return -1;
  if (!pl_start || !pl_end || !row_pl || !row_seg || !row_dir || !row_f || !row_bnd || !status || !seg || !xy) return -1;
  if (!gi::polylines_ok(vtx, nv, pl_off, npl) || !gi::walk_rows_ok(pl_off, npl, n, row_pl, row_seg)) return -1;
  std::vector<uint32_t> blk;
  if (form == gi::WALK_F_LINE_LDS) {  // rows grouped by polyline (ascending), chunks of one block each
    for (uint64_t i = 0; i < n;) {
      const uint32_t p = row_pl[i];
      if (i && p < row_pl[i - 1]) return -1;
      if (pl_off[p + 1] - pl_off[p] > EG3D_PROBE_LDS_VTX) return -1;  // (the caller leaves such polylines out)
      uint64_t e = i;
      while (e < n && row_pl[e] == p && e - i < 256) e++;
      blk.insert(blk.end(), {p, (uint32_t)i, (uint32_t)e});
      i = e;
    }
  }
  DevBuf dv, dpo, dps, dpe, drp, drs, drd, drf, drb, dst, dsg, dxy, dblk;
  PT(dv.up(vtx, (nv + 1) * 8));
  PT(dpo.up(pl_off, ((size_t)npl + 1) * 4));
  PT(dps.up(pl_start, (size_t)npl * 4));
  PT(dpe.up(pl_end, (size_t)npl * 4));
  PT(drp.up(row_pl, n * 4));
  PT(drs.up(row_seg, n * 4));
  PT(drd.up(row_dir, n * 4));
  PT(drf.up(row_f, n * 32));
  PT(drb.up(row_bnd, n));
  PT(dst.up(status, n * 4));  // (the outputs go up too: the sentinel the caller filled them with)
  PT(dsg.up(seg, n * 4));
  PT(dxy.up(xy, n * 8));
  WalkTab t = {dv.as<f2>(),       dpo.as<uint32_t>(), dps.as<uint32_t>(), dpe.as<uint32_t>(), drp.as<uint32_t>(), drs.as<uint32_t>(),
               drd.as<uint32_t>(), drf.as<float>(),    drb.as<uint8_t>(),  dst.as<uint32_t>(), dsg.as<uint32_t>(), dxy.as<float>()};
  if (form == gi::WALK_F_LINE_LDS) {
    PT(dblk.up(blk.data(), blk.size() * 4));
    hipLaunchKernelGGL(k_probe_walk_lds, dim3((unsigned)(blk.size() / 3)), dim3(256), 0, 0, dblk.as<uint32_t>(), t);
  } else {
    hipLaunchKernelGGL(k_probe_walk, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, form, n, t);
  }
  PT_LAUNCH();
  PT(hipDeviceSynchronize());
  PT(dst.down(status, n * 4));
  PT(dsg.down(seg, n * 4));
  PT(dxy.down(xy, n * 8));
  return 0;
}

__global__ void __launch_bounds__(256) k_probe_seg(int mode, uint64_t n, const float* in, uint32_t* r, float* o) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t ri = r[i];
  float oi[2] = {o[2 * i], o[2 * i + 1]};
  gi::seg_item(mode, in + 8 * i, ri, oi);
  r[i] = ri;
  o[2 * i] = oi[0];
  o[2 * i + 1] = oi[1];
}
extern "C" int eg3d_probe_seg(int mode, uint64_t n, const float* in, uint32_t* r, float* o) {
  if (mode < 0 || mode >= gi::SEG_N_MODES || !n || n > 0x7fffffffull || !in || !r || !o) return -1;
  for (uint64_t i = 0; i < 8 * n; i++)
    if (!gi::finite_f(in[i])) return -1;
  DevBuf di, dr, dout;
  PT(di.up(in, n * 32));
  PT(dr.up(r, n * 4));
  PT(dout.up(o, n * 8));
  hipLaunchKernelGGL(k_probe_seg, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, mode, n, di.as<float>(), dr.as<uint32_t>(),
                     dout.as<float>());
  PT_LAUNCH();
  PT(hipDeviceSynchronize());
  PT(dr.down(r, n * 4));
  PT(dout.down(o, n * 8));
  return 0;
}

__global__ void __launch_bounds__(256) k_probe_cells(int mode, uint64_t n, const float* in, const int32_t* dims, int32_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t o[4] = {out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]};
  gi::cell_item(mode, in + 3 * i, dims + 4 * i, o);
  for (int k = 0; k < 4; k++) out[4 * i + k] = o[k];
}
extern "C" int eg3d_probe_cells(int mode, uint64_t n, const float* in, const int32_t* dims, int32_t* out) {
  if (mode < 0 || mode >= gi::CELL_N_MODES || !n || n > 0x7fffffffull || !in || !dims || !out) return -1;
  for (uint64_t i = 0; i < n; i++) {
    if (!gi::finite_f(in[3 * i]) || !gi::finite_f(in[3 * i + 1]) || !gi::finite_f(in[3 * i + 2]) || !(in[3 * i] > 0.0f)) return -1;
    if (mode == gi::CELL_M_WINDOW && (dims[4 * i] < 1 || dims[4 * i + 1] < 1 || dims[4 * i + 2] < 1 || dims[4 * i + 3] < 1)) return -1;
  }
  DevBuf di, dd, dout;
  PT(di.up(in, n * 12));
  PT(dd.up(dims, n * 16));
  PT(dout.up(out, n * 16));
  hipLaunchKernelGGL(k_probe_cells, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, mode, n, di.as<float>(), dd.as<int32_t>(),
                     dout.as<int32_t>());
  PT_LAUNCH();
  PT(hipDeviceSynchronize());
  PT(dout.down(out, n * 16));
  return 0;
}

struct ClosestTab {
  const f2* vtx;
  const uint32_t* pl_off;
  const float* bb;
  const uint32_t* bb_off;
  const uint32_t *row_pl, *row_s0, *row_s1;
  const float* q;
  float* d;
  uint32_t* seg;
  float* xy;
};
__global__ void __launch_bounds__(256) k_probe_closest(int mode, uint64_t n, ClosestTab t) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = t.row_pl[i];
  PlRef pl;
  pl.v = t.vtx + t.pl_off[p];
  pl.n = t.pl_off[p + 1] - t.pl_off[p];
  pl.start = 0;
  pl.end = 1;
  pl.bb = mode == gi::CLOSEST_M_PRUNED ? t.bb + 4 * (size_t)t.bb_off[p] : nullptr;
  PlPt o;
  o.seg = t.seg[i];
  o.x = t.xy[2 * i];
  o.y = t.xy[2 * i + 1];
  t.d[i] = gi::closest_item(mode, pl, t.q[2 * i], t.q[2 * i + 1], t.row_s0[i], t.row_s1[i], o);
  t.seg[i] = o.seg;
  t.xy[2 * i] = o.x;
  t.xy[2 * i + 1] = o.y;
}
extern "C" int eg3d_probe_closest(int mode, const float* vtx, uint64_t nv, const uint32_t* pl_off, uint32_t npl, const float* bb,
                                  uint64_t nbb, const uint32_t* bb_off, uint64_t n, const uint32_t* row_pl, const uint32_t* row_s0,
                                  const uint32_t* row_s1, const float* q, float* d, uint32_t* seg, float* xy) {
  if (mode < 0 || mode >= gi::CLOSEST_N_MODES || !n || n > 0x7fffffffull || nv > 0x7fffffffull) return -1;
  if (!bb || !bb_off || !row_pl || !row_s0 || !row_s1 || !q || !d || !seg || !xy) return -1;
  if (!gi::polylines_ok(vtx, nv, pl_off, npl) || !gi::closest_rows_ok(pl_off, npl, bb_off, nbb, n, row_pl, row_s0, row_s1)) return -1;
  DevBuf dv, dpo, dbb, dbo, drp, d0, d1, dq, dd, dsg, dxy;
  PT(dv.up(vtx, (nv + 1) * 8));
  PT(dpo.up(pl_off, ((size_t)npl + 1) * 4));
  PT(dbb.up(bb, nbb * 16));
  PT(dbo.up(bb_off, ((size_t)npl + 1) * 4));
  PT(drp.up(row_pl, n * 4));
  PT(d0.up(row_s0, n * 4));
  PT(d1.up(row_s1, n * 4));
  PT(dq.up(q, n * 8));
  PT(dd.up(d, n * 4));
  PT(dsg.up(seg, n * 4));
  PT(dxy.up(xy, n * 8));
  ClosestTab t = {dv.as<f2>(),        dpo.as<uint32_t>(), dbb.as<float>(), dbo.as<uint32_t>(), drp.as<uint32_t>(), d0.as<uint32_t>(),
                  d1.as<uint32_t>(), dq.as<float>(),     dd.as<float>(),  dsg.as<uint32_t>(), dxy.as<float>()};
  hipLaunchKernelGGL(k_probe_closest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, mode, n, t);
  PT_LAUNCH();
  PT(hipDeviceSynchronize());
  PT(dd.down(d, n * 4));
  PT(dsg.down(seg, n * 4));
  PT(dxy.down(xy, n * 8));
  return 0;
}

__global__ void __launch_bounds__(256) k_probe_epiline(uint64_t n, const double* F, const uint8_t* valid, const float* xy, int32_t* ok,
                                                       float* line) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float l[3] = {line[3 * i], line[3 * i + 1], line[3 * i + 2]};
  ok[i] = gi::epiline_item(F + 9 * i, valid + i, xy[2 * i], xy[2 * i + 1], l);
  for (int k = 0; k < 3; k++) line[3 * i + k] = l[k];
}
extern "C" int eg3d_probe_epiline(uint64_t n, const double* F, const uint8_t* valid, const float* xy, int32_t* ok, float* line) {
  if (!n || n > 0x7fffffffull || !F || !valid || !xy || !ok || !line) return -1;
  DevBuf dF, dval, dxy, dok, dl;
  PT(dF.up(F, n * 72));
  PT(dval.up(valid, n));
  PT(dxy.up(xy, n * 8));
  PT(dok.up(ok, n * 4));
  PT(dl.up(line, n * 12));
  hipLaunchKernelGGL(k_probe_epiline, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, dF.as<double>(), dval.as<uint8_t>(),
                     dxy.as<float>(), dok.as<int32_t>(), dl.as<float>());
  PT_LAUNCH();
  PT(hipDeviceSynchronize());
  PT(dok.down(ok, n * 4));
  PT(dl.down(line, n * 12));
  return 0;
}
