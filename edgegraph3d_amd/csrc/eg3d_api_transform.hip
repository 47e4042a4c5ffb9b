// eg3d_api_transform.hip — a 4 x 4 transform applied to the points of a cloud (include/eg3d_transform.h): the host side
// of K16
#include <cmath>

#include "eg3d_api_internal.h"
#include "../../include/eg3d_transform.h"

// The checks every entry point makes before it touches the device: the struct, the context, T — finite in FP64 and after
// the conversion to FP32 (a finite double above FLT_MAX becomes an infinity) — and M, the converted matrix.
static int check_call(const char* who, const eg3d_ctx* c, const double* T, const eg3d_transform_stats* stats, K16Mat* M) {
  if (stats) BUF_TRY(check_struct_size(who, "eg3d_transform_stats", stats->struct_size, sizeof(eg3d_transform_stats)));
  if (!c || !T) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      M->m[i][j] = (float)T[4 * i + j];
      if (!std::isfinite(T[4 * i + j]) || !std::isfinite(M->m[i][j])) {
        g_err = std::string(who) + ": T[" + std::to_string(4 * i + j) + "] is not finite (as a double or as a float)";
        return EG3D_ERR_TRANSFORM_NONFINITE;
      }
    }
  return EG3D_OK;
}

static void give_stats(eg3d_transform_stats* stats, eg3d_transform_stats s) {
  if (!stats) return;
  s.struct_size = (uint32_t)sizeof(eg3d_transform_stats);
  *stats = s;
}

// The call proper, on arrays that are on the device: the counts zeroed, the kernel, one read-back.
static int transform_cloud(eg3d_ctx* c, const K16Mat& M, const float* X, uint64_t n, const uint8_t* keep, float* X_out,
                           eg3d_transform_stats* s) {
  hipStream_t st = c->stream;
  BUF_TRY(c->k16_ctr.ensure(2 * sizeof(unsigned long long)));
  unsigned long long* ctr = c->k16_ctr.as<unsigned long long>();  // [0] points the mask drops, [1] non-finite results
  HIP_TRY(hipMemsetAsync(ctr, 0, 2 * sizeof(unsigned long long), st));
  HIP_TRY(hipEventRecord(c->ea[0], st));
  launch_k16_transform(st, M, X, n, keep, X_out, ctr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  unsigned long long back[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(back, ctr, sizeof(back), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  s->n_points = n;
  s->n_transformed = n - back[0];
  s->n_nonfinite = back[1];
  HIP_TRY(hipEventElapsedTime(&s->ms_kernel, c->ea[0], c->eb[0]));
  return EG3D_OK;
}

extern "C" int eg3d_transform_device(eg3d_ctx* c, const eg3d_device_edgepoints* cloud, const double* T, const uint8_t* keep_dev,
                                     float* X_out_dev, eg3d_transform_stats* stats) {
  const char* who = "eg3d_transform_device";
  K16Mat M;
  BUF_TRY(check_call(who, c, T, stats, &M));
  eg3d_device_edgepoints d;
  if (cloud)
    d = *cloud;
  else
    BUF_TRY(eg3d_last_device_output(c, &d));
  BUF_TRY(check_cloud(&d, who, false));
  eg3d_transform_stats s{};
  if (!d.n_points) {
    give_stats(stats, s);
    return EG3D_OK;
  }
  float* X = const_cast<float*>(d.X);  // (in place: the view is const, the memory is the caller's or this context's)
  float* out = X_out_dev ? X_out_dev : X;
  if (out != X) {
    const uintptr_t a = (uintptr_t)X, b = (uintptr_t)out, len = (uintptr_t)d.n_points * 12u;
    if (a < b + len && b < a + len) {
      g_err = std::string(who) + ": X_out_dev overlaps the cloud's X without being it";
      return EG3D_ERR_TRANSFORM_OVERLAP;
    }
  }
  HIP_TRY(hipSetDevice(c->device));
  BUF_TRY(transform_cloud(c, M, X, d.n_points, keep_dev, out, &s));
  give_stats(stats, s);
  return EG3D_OK;
}

extern "C" int eg3d_transform_points(eg3d_ctx* c, const double* T, const float* X_host, uint64_t n, float* X_out_host,
                                     eg3d_transform_stats* stats) {
  const char* who = "eg3d_transform_points";
  K16Mat M;
  BUF_TRY(check_call(who, c, T, stats, &M));
  eg3d_transform_stats s{};
  if (!n) {
    give_stats(stats, s);
    return EG3D_OK;
  }
  if (!X_host || !X_out_host) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  const auto w0 = std::chrono::steady_clock::now();
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  BUF_TRY(upload(c->k16_X, X_host, 3 * n, st));
  BUF_TRY(transform_cloud(c, M, c->k16_X.as<float>(), n, nullptr, c->k16_X.as<float>(), &s));
  HIP_TRY(hipMemcpyAsync(X_out_host, c->k16_X.p, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const float wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
  s.ms_copy = std::max(0.f, wall - s.ms_kernel);
  give_stats(stats, s);
  return EG3D_OK;
}
