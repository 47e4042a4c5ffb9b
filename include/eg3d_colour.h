/*
 * eg3d_colour.h — the colours of an edge-point cloud from the source images, K15 (libeg3d.so, libeg3d_dlt4x4.so; the
 * result does not depend on the DLT form). What the reference's json_to_ply computes for its coloured point cloud
 * (io/output/output_point_cloud.cpp:65-105, 127-170), on a cloud that stays where it was built: one RGB triple per point.
 *
 * Sample. For an observation (px, py) in view v, whose image has W columns and H rows (RGB8 interleaved, row-major,
 * channel 0 = red): x = (int)px, y = (int)py (truncation toward zero, NOT floor); a = px - (float)x, c = py - (float)y in
 * FP32 (for px = -0.5: x = 0, a = -0.5, the weights extrapolate); x0 = R(x, W), x1 = R(x + 1, W), y0 = R(y, H),
 * y1 = R(y + 1, H) with R = the reflection without repeated border (p in [0, len) stays; len == 1 gives 0; otherwise
 * p < 0 -> -p, p >= len -> 2 len - 2 - p, until p is inside); per channel
 *   s = (I[y0][x0] (1 - a) + I[y0][x1] a) (1 - c) + (I[y1][x0] (1 - a) + I[y1][x1] a) c
 * with every product and sum in FP32 in this order, no FMA; q = s rounded to the nearest int, ties to even; the channel
 * byte is the low 8 bits of q (256 -> 0, -1 -> 255).
 *
 * Mix. Per channel the bytes of the point's n observations are summed and divided: the colour is the INTEGER sum / n.
 * The reference sums in double, divides by float(n) and prints int(.). That is the same number. The sums are integers
 * below 255 * 2^15 < 2^23 and n <= 32 767 (the cap eg3d_triangulate puts on a list), so sum and n are exact in FP32 and in
 * double, in any summation order. Write sum = k n + r with 0 <= r < n. If r == 0 the quotient is the integer k <= 255,
 * representable, and the division returns it. Otherwise the true quotient k + r / n lies at least 1 / n > 2^-15 from k and
 * from k + 1, while the division rounds by at most half an ulp of a value below 256: 2^-17 in FP32, less in double. The
 * rounded quotient therefore stays strictly inside (k, k + 1) and int(.) gives k = sum / n, the integer division.
 * Deviation: a point with n == 0 is undefined behaviour in the reference (0 / 0 cast to int). Here it gets (0, 0, 0),
 * EG3D_COLOUR_FLAG_EMPTY in flags, and is counted in n_empty.
 *
 * Images belong to the context they were uploaded to: they are freed by eg3d_release_images, by the next upload, or with
 * the context. A clone (eg3d_clone) does NOT inherit them: it is refused until it uploads its own. PNG files are read by
 * eg3d_host_png_read_rgb (include/eg3d_host_colour.h); JPEG is not read by this project.
 *
 * Checks, made ON THE DEVICE before any value is used as an index (the contract of eg3d_gn_filter_device). The call fails
 * with EG3D_ERR_ARG, and its outputs are unspecified, on: offsets that do not ascend within [0, n_obs] (any point); and,
 * for the points the mask keeps: a list of more than 32 767 observations, a view id outside the context's rig, a view
 * without an image, a coordinate that is not finite or whose magnitude is >= 1e7 (the scene's bound; it keeps (int)px
 * defined). Observations of points the mask drops are not held to these. No images uploaded, and a stats struct whose
 * struct_size is smaller than this library's, are refused before anything is written. After a refused call the context
 * serves a valid one. n_points == 0 is EG3D_OK.
 */
#ifndef EG3D_COLOUR_H_
#define EG3D_COLOUR_H_
#include "eg3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EG3D_COLOUR_FLAG_EMPTY 1u /* a kept point without observations: colour (0, 0, 0) */
#define EG3D_COLOUR_MAX_IMAGE_SIDE 32768

typedef struct eg3d_colour_stats {
  uint32_t struct_size;   /* sizeof(eg3d_colour_stats), set by the caller */
  uint32_t n_images;      /* views of the context that have an image */
  uint64_t n_points;      /* points in */
  uint64_t n_coloured;    /* kept points with at least one observation */
  uint64_t n_empty;       /* kept points without observations */
  uint64_t n_obs_sampled; /* observations of the kept points */
  float ms_sample;        /* the sampling pass (over ALL observations of the cloud) */
  float ms_mix;           /* the checks of the offsets and the per-point means */
  float ms_copy;          /* eg3d_colour_points: the caller's arrays to the device and the colours back (wall time) */
} eg3d_colour_stats;

/* n_views must equal the context's; width[v] x height[v] is the size of rgb[v] (RGB8 interleaved, row-major, 1 .. 32 768
 * per side, each view its own); rgb[v] == NULL: view v has no image (its width and height are ignored). A second upload
 * replaces the first. */
int eg3d_upload_images(eg3d_ctx* ctx, int n_views, const int32_t* width, const int32_t* height, const uint8_t* const* rgb);
int eg3d_release_images(eg3d_ctx* ctx);

/* device-resident: cloud == NULL -> the context's last device output (which must be `complete`); 64-bit offsets without
 * a sentinel, the alignment contract of eg3d_gn_filter_device; keep_dev [n_points] may be NULL (all kept); rgb_dev
 * [n_points][3]; flags_dev [n_points] may be NULL; stats may be NULL. A point with keep == 0 gets (0, 0, 0) and flag 0. */
int eg3d_colour_device(eg3d_ctx* ctx, const eg3d_device_edgepoints* cloud, const uint8_t* keep_dev, uint8_t* rgb_dev,
                       uint8_t* flags_dev, eg3d_colour_stats* stats);

/* host arrays; obs_off [n_points + 1] as in eg3d_gn_filter; keep [n_points] may be NULL; rgb_out [n_points][3];
 * flags_out [n_points] may be NULL; stats may be NULL */
int eg3d_colour_points(eg3d_ctx* ctx, uint64_t n_points, const uint32_t* obs_off, const int32_t* obs_view, const float* obs_xy,
                       const uint8_t* keep, uint8_t* rgb_out, uint8_t* flags_out, eg3d_colour_stats* stats);

#ifdef __cplusplus
}
#endif
#endif
