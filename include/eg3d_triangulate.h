/*
 * eg3d_triangulate.h — FP64 triangulation of caller-supplied tracks on the device, K14 (libeg3d.so, libeg3d_dlt4x4.so).
 * The arithmetic every stage of the library rests on, as an entry point of its own: one observation list per track in,
 * one point and one verdict per track out, bit for bit what the reference computes on the same list.
 *
 *   EG3D_TRI_FROM_SCRATCH  compute_3d_point_coords / em_estimate3Dpositions (utils/geometry/triangulation.cpp:178-323,
 *                          468-481): the 2-view DLT on (the first entry with the minimal view id, the LAST entry) — with the
 *                          system of this library's OpenCV form, eg3d_dlt_rows() — then Gauss-Newton over all entries.
 *   EG3D_TRI_REFINE        the solve of em_add_new_observation_to_3Dpositions (:347-466): Gauss-Newton from the stored
 *                          float point X0 over all entries, no DLT.
 *
 * Per track: valid[i] = the solve was accepted; X_out[i] = the (float) of the accepted FP64 solution. A track that is not
 * valid gets X0[i] in EG3D_TRI_REFINE and +0.0 in EG3D_TRI_FROM_SCRATCH. flags[i] (optional): EG3D_TRI_FLAG_*.
 *
 * Checks, made ON THE DEVICE before any value is used as an index (the contract of eg3d_gn_filter_device): a view id
 * outside the context's rig, offsets that do not ascend within [0, n_obs], and a list of more than 32 767 observations
 * fail the call with EG3D_ERR_ARG; the outputs are then unspecified. A stats struct whose struct_size is smaller than this
 * library's and an unknown mode are refused before anything is written. n_tracks == 0 is EG3D_OK.
 *
 * The solver reads 16-byte observation records; the call converts the caller's arrays into them batch by batch, cutting
 * its range at track boundaries so that the records of a batch stay under a budget in observations
 * (EG3D_TRI_STAGE_OBS in the environment, read at the call; default 16 777 216 = 256 MiB). A single track larger than the
 * budget runs alone. The result does not depend on the budget.
 */
#ifndef EG3D_TRIANGULATE_H_
#define EG3D_TRIANGULATE_H_
#include "eg3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EG3D_TRI_FROM_SCRATCH 0
#define EG3D_TRI_REFINE 1
#define EG3D_TRI_FLAG_SHORT 1u      /* fewer than 2 observations: valid = 0, no arithmetic (triangulation.cpp:468-481) */
#define EG3D_TRI_FLAG_DEGENERATE 2u /* both DLT entries name the same view; the solve still runs, as in the reference */

typedef struct eg3d_tri_stats {
  uint32_t struct_size; /* sizeof(eg3d_tri_stats), set by the caller */
  uint32_t n_batches;
  uint64_t n_tracks;
  uint64_t n_valid;
  uint64_t n_short;
  uint64_t n_degenerate;
  float ms_kernel; /* the batches: per batch the conversion into records and the solve kernel */
  float ms_stage;  /* the checks of the offsets and the cut into batches */
  float ms_copy;   /* eg3d_triangulate: the caller's arrays to the device and the results back (wall time) */
} eg3d_tri_stats;

/* host arrays; view ids index ctx's cameras; obs_off [n_tracks + 1] as in eg3d_gn_filter; X0 [n_tracks][3], NULL in
 * EG3D_TRI_FROM_SCRATCH; X_out [n_tracks][3]; valid [n_tracks]; flags [n_tracks], may be NULL; stats may be NULL */
int eg3d_triangulate(eg3d_ctx* ctx, int mode, uint64_t n_tracks, const uint32_t* obs_off, const int32_t* obs_view,
                     const float* obs_xy, const float* X0, float* X_out, uint8_t* valid, uint8_t* flags, eg3d_tri_stats* stats);

/* device-resident: cloud == NULL -> the context's last device output (which must be `complete`); 64-bit offsets without
 * a sentinel, the alignment contract of eg3d_gn_filter_device; X0 is cloud->X; X_out_dev [n_points][3] may alias cloud->X;
 * valid_dev [n_points]; flags_dev [n_points], may be NULL. X_out_dev and valid_dev plug into eg3d_compact_device. */
int eg3d_triangulate_device(eg3d_ctx* ctx, int mode, const eg3d_device_edgepoints* cloud, float* X_out_dev, uint8_t* valid_dev,
                            uint8_t* flags_dev, eg3d_tri_stats* stats);

#ifdef __cplusplus
}
#endif
#endif
