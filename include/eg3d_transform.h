/*
 * eg3d_transform.h — a 4 x 4 transform applied to the points of a cloud where it lies, K16 (libeg3d.so,
 * libeg3d_dlt4x4.so; the result does not depend on the DLT form). The point step of the reference's
 * coordinate_system_transform (transform_3d_point, coordinate_system_transform/transform_coordinate_system.cpp:152-155):
 * a cloud built and left in HBM is brought into the frame of known camera centres without crossing to the host.
 *
 * T is the row-major FP64 4 x 4 that eg3d_host_similarity_fit returns (include/eg3d_host_transform.h; the fit itself stays
 * on the host: tens to hundreds of cameras). It is converted element by element to FP32, M[i][j] = (float)T[4 i + j], and
 * every kept point becomes
 *   h[j] = ((M[j][0] x + M[j][1] y) + M[j][2] z) + M[j][3] 1.0f,  j = 0 .. 3;   p' = (h[0] / h[3], h[1] / h[3], h[2] / h[3])
 * in FP32, no FMA, correctly rounded division: bit for bit what eg3d_host_transform_points computes, which restates the
 * glm the reference vendors (pinned: tests/test_transform_glm_pin.py). A point the mask drops keeps its bits.
 *
 * Only the X array of the cloud is read, and only X_out is written (X itself when X_out is NULL): offsets, observations
 * and the polyline arrays are untouched, so the cloud still feeds eg3d_compact_device, eg3d_colour_device, the filters
 * and a fetch. Neither array needs more than a float's alignment.
 *
 * Refused BEFORE anything is launched or written, each with its own code: a stats struct smaller than the library's, a
 * null context or T, a cloud without X (EG3D_ERR_ARG); an entry of T that is not finite — after the conversion to FP32
 * as well — (EG3D_ERR_TRANSFORM_NONFINITE); an X_out that overlaps X without being X (EG3D_ERR_TRANSFORM_OVERLAP).
 * n_points == 0 is EG3D_OK. A non-finite RESULT is no refusal: such points are counted in n_nonfinite.
 */
#ifndef EG3D_TRANSFORM_H_
#define EG3D_TRANSFORM_H_
#include "eg3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EG3D_ERR_TRANSFORM_NONFINITE -16
#define EG3D_ERR_TRANSFORM_OVERLAP -17

typedef struct eg3d_transform_stats {
  uint32_t struct_size;   /* sizeof(eg3d_transform_stats), set by the caller */
  uint32_t reserved;
  uint64_t n_points;      /* points in */
  uint64_t n_transformed; /* points the mask keeps */
  uint64_t n_nonfinite;   /* of those: results with a NaN or infinite coordinate */
  float ms_kernel;
  float ms_copy;          /* eg3d_transform_points: the caller's arrays to the device and back (wall time) */
} eg3d_transform_stats;

/* device-resident: cloud == NULL -> the context's last device output (which must be `complete`); keep_dev [n_points] may
 * be NULL (all kept); X_out_dev [n_points][3] may be NULL (in place: the cloud's X is overwritten); stats may be NULL */
int eg3d_transform_device(eg3d_ctx* ctx, const eg3d_device_edgepoints* cloud, const double* T_f64, const uint8_t* keep_dev,
                          float* X_out_dev, eg3d_transform_stats* stats);

/* host arrays: X_host, X_out_host [n][3] (may be the same array); stats may be NULL */
int eg3d_transform_points(eg3d_ctx* ctx, const double* T_f64, const float* X_host, uint64_t n, float* X_out_host,
                          eg3d_transform_stats* stats);

#ifdef __cplusplus
}
#endif
#endif
