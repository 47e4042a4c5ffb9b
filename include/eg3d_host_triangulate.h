/*
 * eg3d_host_triangulate.h — the host statement of include/eg3d_triangulate.h (libeg3d_host.so): the same call, track
 * after track, compiled from the same functions the kernels are built from (triangulate_array, gauss_newton_f64), usable
 * without a GPU. Both forms of cv::triangulatePoints' system live in the one host library: dlt_rows = 3 is the 6x4 system
 * (libeg3d.so), 2 the 4x4 one (libeg3d_dlt4x4.so).
 *
 * Returns 0, or -1 for bad arguments: dlt_rows other than 2 and 3, an unknown mode, a NULL array that is needed, n_views
 * < 1, offsets that do not ascend, a list of more than 32 767 observations, a view id outside [0, n_views). Everything is
 * checked before anything is computed or written. Tracks are independent: n_threads splits them, and the bytes do not
 * depend on it.
 */
#ifndef EG3D_HOST_TRIANGULATE_H_
#define EG3D_HOST_TRIANGULATE_H_
#include "eg3d_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cam_P [n_views][16]; mode, obs_off [n_tracks + 1], obs_view, obs_xy, X0 (NULL in mode 0), X_out, valid, flags (may be
 * NULL): as eg3d_triangulate */
int eg3d_host_triangulate(int dlt_rows, const float* cam_P, int n_views, int mode, uint64_t n_tracks, const uint32_t* obs_off,
                          const int32_t* obs_view, const float* obs_xy, const float* X0, int n_threads, float* X_out,
                          uint8_t* valid, uint8_t* flags);

#ifdef __cplusplus
}
#endif
#endif
