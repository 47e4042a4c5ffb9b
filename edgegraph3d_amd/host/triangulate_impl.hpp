// triangulate_impl.hpp — the per-track body of eg3d_host_triangulate, written once and compiled twice: triangulate.cpp
// includes it with the 6x4 DLT system (EG3D_DLT_ROWS = 3, namespace eg3d), triangulate_dlt4x4.cpp with the 4x4 one
// (EG3D_DLT_ROWS = 2) and every name of the kernels' headers moved into a namespace of its own, so that the two
// compilations of dlt2 / svd4_smallest_v never meet as one inline function.
//
// The track is copied into Obs records and handed to triangulate_array / gauss_newton_f64 of eg3d_dev_tri.h — the
// functions the kernels are built from. KEEP = 0: the update pass recomputes its rows (the same values in the same
// order; no per-track array of kept rows).
#include <vector>

#include "eg3d_dev_tri.h"

namespace eg3d {

// rows [a, b) of obs_view / obs_xy, already checked; X0 = the track's start point (mode 1) or null (mode 0)
inline void host_triangulate_track(const float* cam_P, int mode, const int32_t* obs_view, const float* obs_xy, uint32_t a,
                                   uint32_t b, const float* X0, std::vector<Obs>& rec, float* X_out, uint8_t* valid,
                                   uint8_t* flags) {
  const int n = (int)(b - a);
  float X[3] = {mode == 1 ? X0[0] : 0.f, mode == 1 ? X0[1] : 0.f, mode == 1 ? X0[2] : 0.f};
  uint32_t fl = 0;
  bool ok = false;
  if (n < 2) {
    fl |= 1u;  // EG3D_TRI_FLAG_SHORT
  } else {
    rec.resize((size_t)n);
    for (int k = 0; k < n; k++) {
      Obs& o = rec[(size_t)k];
      o.view = (uint32_t)obs_view[a + (uint32_t)k];
      o.pl = 0;
      o.seg = 0;
      o.x = obs_xy[2 * (size_t)(a + (uint32_t)k)];
      o.y = obs_xy[2 * (size_t)(a + (uint32_t)k) + 1];
    }
    float Xs[3] = {0.f, 0.f, 0.f};
    if (mode == 0) {
      uint32_t tf = 0;
      ok = triangulate_array<0>(cam_P, rec.data(), n, Xs, tf);
      if (tf & 16u) fl |= 2u;  // EG3D_TRI_FLAG_DEGENERATE
    } else {
      ArrayCursor c;
      c.a = rec.data();
      c.n = n;
      c.extra = nullptr;
      c.i = 0;
      const double X0d[3] = {(double)X0[0], (double)X0[1], (double)X0[2]};
      ok = gauss_newton_f64<ArrayCursor, 0>(cam_P, c, X0d, Xs);
    }
    if (ok) {
      X[0] = Xs[0];
      X[1] = Xs[1];
      X[2] = Xs[2];
    }
  }
  X_out[0] = X[0];
  X_out[1] = X[1];
  X_out[2] = X[2];
  *valid = ok ? 1 : 0;
  if (flags) *flags = (uint8_t)fl;
}

inline void host_triangulate_tracks(const float* cam_P, int mode, uint64_t n_tracks, const uint32_t* obs_off,
                                    const int32_t* obs_view, const float* obs_xy, const float* X0, int n_threads, float* X_out,
                                    uint8_t* valid, uint8_t* flags) {
#pragma omp parallel num_threads(n_threads > 1 ? n_threads : 1)
  {
    std::vector<Obs> rec;
#pragma omp for schedule(dynamic, 64)
    for (int64_t i = 0; i < (int64_t)n_tracks; i++)
      host_triangulate_track(cam_P, mode, obs_view, obs_xy, obs_off[i], obs_off[i + 1], X0 ? X0 + 3 * i : nullptr, rec,
                             X_out + 3 * i, valid + i, flags ? flags + i : nullptr);
  }
}

}  // namespace eg3d
