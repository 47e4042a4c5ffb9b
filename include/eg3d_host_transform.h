/*
 * eg3d_host_transform.h — bring a reconstruction into the frame of known camera centres (libeg3d_host.so). No GPU.
 * What the reference's coordinate_system_transform computes (src/coordinate_system_transform/
 * transform_coordinate_system.cpp; line numbers below are that file's): a similarity fitted to the camera centres, applied
 * to the cameras and to every point.
 *
 * Null cameras (:101-106). A camera whose centre AND whole rotation are exactly 0.0 (a view without a pose). It takes no
 * part in the fit, is never updated and adds nothing to the error sum, but its triple in the poses file is read.
 *
 * Poses file (:116-135). One "x y z" triple per camera, in camera order, separated by any white space, read as doubles.
 * Deviation: the reference reads on past the end of a short or unreadable file and fits to whatever its variables then
 * hold. Here that is refused (EG3D_TRANSFORM_ERR_SHORT, EG3D_TRANSFORM_ERR_FILE).
 *
 * Fit (:137-150), FP64, on the non-null cameras. UNPINNED: the reference calls Eigen::umeyama(src, dst, true); Eigen is
 * neither vendored by the reference nor available to this project, so the statement below follows Umeyama's paper
 * ("Least-squares estimation of transformation parameters between two point patterns", PAMI 13(4), 1991) and Eigen's
 * documented algorithm, and agrees with Eigen's result up to rounding, not bit for bit:
 *   means of src and dst (sum in camera order, times 1 / n); src_var = (sum of the squared norms of the demeaned src) / n;
 *   sigma = (1 / n) dst_demean src_demean^T (each of the 9 sums in camera order);
 *   sigma = U diag(d) V^T by a one-sided Jacobi on the 3 x 3 matrix: pairs (0,1), (0,2), (1,2) in this order, at most 30
 *   sweeps, a pair is left alone when |<a_p, a_q>| <= 2^-52 sqrt(|a_p|^2 |a_q|^2), sqrt(1 + z z) and never hypot
 *   (csrc/eg3d_fund_core.h says why), singular values sorted descending (the earlier column first on a tie);
 *   S = diag(1, 1, s) with s = -1 when det(U) det(V) < 0 (the target is a mirror image: `reflection`), else +1;
 *   R = U S V^T;  c = (d0 + d1 + s d2) / src_var;  t = dst_mean - c R src_mean;  T = [c R, t; 0 0 0 1], row-major.
 * A singular value <= 1e-12 d0 counts as zero. Its column of U is completed to an orthonormal basis with the handedness
 * of V, so that det(U) det(V) > 0 (a planar set of centres, rank 2, has its unique answer — a plane is its own mirror
 * image, and no reflection is reported for it). With rank < 2 (collinear or coincident centres in src or dst)
 * the rotation about the line is not determined: the call still returns a proper rotation and sets `rank_deficient`.
 * Compiled with -ffp-contract=off like the rest of the library.
 *
 * Conversion (:245-248): M[i][j] = (float)T[4 i + j]. Everything below is FP32, no FMA, and PINNED: it restates the glm
 * 0.9.6 the reference vendors, operation by operation (tests/test_transform_glm_pin.py holds it to that glm bit for bit).
 *
 * Points (:152-155), vec4(p, 1) * M then the division:
 *   h[j] = ((M[j][0] x + M[j][1] y) + M[j][2] z) + M[j][3] 1.0f,  j = 0 .. 3;   p' = (h[0] / h[3], h[1] / h[3], h[2] / h[3]).
 * The division stays although h[3] is 1 for a fitted T: a non-finite coordinate comes out as the reference's would.
 *
 * Cameras (:157-174), non-null only. With the project's arrays (host/camera_model.hpp: R[3 i + j] = glm rotation[i][j],
 * K = [f 0 ppx; 0 f ppy; 0 0 1] in the top-left of a zero 4 x 4, E = [R t; 0 0 0 1]):
 *   I = glm::inverse(M): the cofactor form of glm/detail/type_mat4x4.inl:37-92, in its evaluation order;
 *   e[i][j] = ((I[0][j] E[i][0] + I[1][j] E[i][1]) + I[2][j] E[i][2]) + I[3][j] E[i][3]      (glm: inverse(M) * E)
 *   P[i][j] = ((e[0][j] K[i][0] + e[1][j] K[i][1]) + e[2][j] K[i][2]) + e[3][j] K[i][3]      (glm: e * K4)
 *   R' = the top-left 3 x 3 of e (it carries the factor 1 / c: not a rotation any more, as in the reference);
 *   t' = (e[0][3], e[1][3], e[2][3]);  C' = the point transform of C.
 * (The reference's `cameraMatrix *= transformation` at :161 is overwritten at :170 and has no effect.) All four fields the
 * reference updates have a stored counterpart here: cameraMatrix = P, rotation = R, translation = t, center = C.
 *
 * Errors (:189-206). sum, a float, over the non-null cameras in order: sum = (float)((double)sum + |C - target|), the norm
 * in FP64 as sqrt((dx dx + dy dy) + dz dz); the result is sum / n_cameras with n_cameras the count of ALL cameras, null
 * ones included (the reference's quirk, kept: DESIGN.md 3, Q16).
 */
#ifndef EG3D_HOST_TRANSFORM_H_
#define EG3D_HOST_TRANSFORM_H_
#include "eg3d_host.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EG3D_TRANSFORM_OK 0
#define EG3D_TRANSFORM_ERR_ARG (-1)        /* a null pointer, a negative count, a stats struct that is too small */
#define EG3D_TRANSFORM_ERR_FEW (-2)        /* fewer than 3 non-null cameras */
#define EG3D_TRANSFORM_ERR_DEGENERATE (-3) /* all source centres are equal: src_var is 0, or <= 1e-28 of their mean squared norm
                                              (what the rounding of the mean leaves of an exact 0) */
#define EG3D_TRANSFORM_ERR_NONFINITE (-4)  /* a NaN or an infinity in a centre that takes part (or in T, where T is input) */
#define EG3D_TRANSFORM_ERR_FILE (-5)       /* the poses file cannot be opened */
#define EG3D_TRANSFORM_ERR_SHORT (-6)      /* the poses file holds fewer than 3 n_cameras numbers */

typedef struct eg3d_similarity_stats {
  uint32_t struct_size;    /* sizeof(eg3d_similarity_stats), set by the caller */
  uint32_t n_used;         /* non-null cameras */
  double scale;            /* c */
  double singular[3];      /* of sigma, descending */
  double src_var;
  uint32_t reflection;     /* det(U) det(V) < 0: S = diag(1, 1, -1) */
  uint32_t rank_deficient; /* fewer than two singular values above 1e-12 d0 */
} eg3d_similarity_stats;

/* out_xyz_f64 [n_cameras][3] */
int eg3d_host_read_camera_poses(const char* path, int n_cameras, double* out_xyz_f64);

/* mask_out [n][1]: 1 where the camera is null (R9 [n][9], C3 [n][3], as the SfM object holds them) */
int eg3d_host_null_cameras(int n, const float* R9, const float* C3, uint8_t* mask_out);

/* src, dst [n][3]; null_mask [n] may be NULL (none); T_out_f64 [16] row-major; stats may be NULL */
int eg3d_host_similarity_fit(int n, const double* src_xyz_f64, const double* dst_xyz_f64, const uint8_t* null_mask,
                             double* T_out_f64, eg3d_similarity_stats* stats);

/* X_f32, X_out_f32 [n][3]; X_out_f32 == X_f32 is allowed (partial overlap is not). T is not checked: a NaN in it gives
 * what the arithmetic gives. */
int eg3d_host_transform_points(const double* T_f64, const float* X_f32, uint64_t n, float* X_out_f32);

/* fpp [n][3] = focal, ppx, ppy (read); R9 [n][9], C3 [n][3], t3 [n][3] (read and written); P16 [n][16] (written); a null
 * camera's entries are left as they are, P16 included. T must be finite (EG3D_TRANSFORM_ERR_NONFINITE). */
int eg3d_host_transform_cameras(const double* T_f64, int n_cameras, const float* fpp, float* R9, float* C3, float* t3, float* P16);

/* the glm operations the camera update is made of, on row-major [4][4] float arrays indexed as glm indexes (m[i][j]):
 * out = glm::inverse(m); out = a * b as glm multiplies. For the pin test. */
int eg3d_host_glm_inverse4(const float* m16, float* out16);
int eg3d_host_glm_mul4(const float* a16, const float* b16, float* out16);

/* C3 [n][3]; null_mask [n] may be NULL; target [n][3]; *error_out = the reference's mean position error (see above) */
int eg3d_host_camera_errors(int n_cameras, const float* C3, const uint8_t* null_mask, const double* target_xyz_f64, float* error_out);

/* ---- on a loaded SfM object (eg3d_sfm_read_json / eg3d_sfm_create) ---- */
/* centres_f64 [n_views][3] = the centres widened to double; null_mask [n_views]; either may be NULL */
int eg3d_sfm_camera_centres(const eg3d_sfm* s, double* centres_f64, uint8_t* null_mask);
#define EG3D_SFM_TRANSFORM_CAMERAS 1
#define EG3D_SFM_TRANSFORM_POINTS 2
/* update_sfmd_transform (:208-216): the cameras and / or all points of `s` (what = a sum of the two bits above), after
 * which eg3d_sfm_write_json writes what the reference's tool writes. Points alone are left to a caller that transforms
 * them elsewhere (on the device) and stores them with eg3d_sfm_set_point_coords. */
int eg3d_sfm_apply_transform(eg3d_sfm* s, const double* T_f64, int what);

#ifdef __cplusplus
}
#endif
#endif
