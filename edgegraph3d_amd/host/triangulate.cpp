// triangulate.cpp — eg3d_host_triangulate (include/eg3d_host_triangulate.h): the sequential statement of K14, track
// after track, from the functions of eg3d_dev_tri.h. This file holds the checks and the 6x4 form of the DLT system;
// triangulate_dlt4x4.cpp compiles the same body (triangulate_impl.hpp) with the 4x4 form.
#include "eg3d_host_triangulate.h"
#include "triangulate_impl.hpp"

// (triangulate_dlt4x4.cpp)
void eg3d_host_triangulate_tracks_dlt4x4(const float* cam_P, int mode, uint64_t n_tracks, const uint32_t* obs_off,
                                         const int32_t* obs_view, const float* obs_xy, const float* X0, int n_threads,
                                         float* X_out, uint8_t* valid, uint8_t* flags);

extern "C" int eg3d_host_triangulate(int dlt_rows, const float* cam_P, int n_views, int mode, uint64_t n_tracks,
                                     const uint32_t* obs_off, const int32_t* obs_view, const float* obs_xy, const float* X0,
                                     int n_threads, float* X_out, uint8_t* valid, uint8_t* flags) {
  if ((dlt_rows != 2 && dlt_rows != 3) || (mode != 0 && mode != 1) || !cam_P || n_views < 1 || n_views > EG3D_MAX_VIEWS) return -1;
  if (!n_tracks) return 0;
  if (!obs_off || !X_out || !valid || (mode == 1 && !X0)) return -1;
  for (uint64_t i = 0; i < n_tracks; i++)
    if (obs_off[i + 1] < obs_off[i] || obs_off[i + 1] - obs_off[i] > 32767u) return -1;
  const uint64_t m = (uint64_t)obs_off[n_tracks] - obs_off[0];
  if (m && (!obs_view || !obs_xy)) return -1;
  for (uint64_t k = obs_off[0]; k < obs_off[n_tracks]; k++)
    if (obs_view[k] < 0 || obs_view[k] >= n_views) return -1;
  if (dlt_rows == 3)
    eg3d::host_triangulate_tracks(cam_P, mode, n_tracks, obs_off, obs_view, obs_xy, X0, n_threads, X_out, valid, flags);
  else
    eg3d_host_triangulate_tracks_dlt4x4(cam_P, mode, n_tracks, obs_off, obs_view, obs_xy, X0, n_threads, X_out, valid, flags);
  return 0;
}
