// triangulate_dlt4x4.cpp — the body of eg3d_host_triangulate with the 4x4 form of cv::triangulatePoints' system
// (EG3D_DLT_ROWS = 2: OpenCV >= 3.2, libeg3d_dlt4x4.so). The rest of the host library compiles eg3d_dev_tri.h with the
// default 6x4 form; here every name of the kernels' headers lives in a namespace of its own, so that the two
// compilations of the inline dlt2 / svd4_smallest_v are two functions to the linker.
#include <stdint.h>
#include <math.h>

#include <vector>

#define EG3D_DLT_ROWS 2
#define eg3d eg3d_dlt4x4
#include "triangulate_impl.hpp"
#undef eg3d

void eg3d_host_triangulate_tracks_dlt4x4(const float* cam_P, int mode, uint64_t n_tracks, const uint32_t* obs_off,
                                         const int32_t* obs_view, const float* obs_xy, const float* X0, int n_threads,
                                         float* X_out, uint8_t* valid, uint8_t* flags) {
  eg3d_dlt4x4::host_triangulate_tracks(cam_P, mode, n_tracks, obs_off, obs_view, obs_xy, X0, n_threads, X_out, valid, flags);
}
