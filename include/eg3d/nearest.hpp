/*
 * eg3d/nearest.hpp — cloud-to-cloud nearest distances where the cloud lies, K18 (libeg3d.so, libeg3d_dlt4x4.so; the
 * result does not depend on the DLT form). The definition, the figures and the error codes are those of
 * include/eg3d/host_nearest.hpp; the bytes are those of eg3d_host_cloud_nearest on host copies of the same arrays.
 *
 * (Why .hpp: two existing tests pin the set of .h files under include/. The text is the C/C++ common subset like every
 * other ABI header and compiles as C99; its registry is _cabi.HPP_HEADERS / _cdefs.MIRRORS_HPP.)
 *
 * An INDEX is a uniform grid over a reference point set, built on the device: a minimum / maximum reduction gives the
 * origin and the extent, a radix sort of (cell key, original index) — x the fastest axis of the key — puts the points in
 * key order, and one pass writes the ascending keys of the occupied cells and their start offsets. A query finds the
 * cells x-1 .. x+1 of one (y, z) row with one binary search and reads their points as one contiguous run.
 *
 * An index belongs to the context that built it: it works on that context's stream and holds its own device memory and
 * the work buffers of the queries made against it. eg3d_destroy does not know the indices of a context: every index is
 * released with eg3d_cloud_index_free, before or after its context is destroyed (freeing touches the index's own memory
 * alone); USING an index whose context is gone is undefined. Calls on one index must not overlap.
 *
 * Refused before anything of the result is written — d2_out, nn_out, *index and stats untouched: a stats struct smaller
 * than the library's, a null context or index, a null array with a count above 0 (EG3D_ERR_ARG); a cloud that is not
 * `complete` or has no X (EG3D_ERR_ARG); an index of another context (EG3D_NEAREST_ERR_FOREIGN); cell, max_dist,
 * thresholds as the host header states (EG3D_NEAREST_ERR_CELL, _MAXDIST, _THRESHOLD); n >= 2^32 (EG3D_ERR_CAPACITY); 2^21
 * cells or more on an axis (EG3D_NEAREST_ERR_EXTENT — the one refusal that follows a launch, the reduction that finds the
 * extent; the others are decided on the host before any). n == 0 is no refusal: an empty index answers "none" to every
 * query, and no query gives figures of an empty set.
 *
 * EG3D_K18_GROUP=1|8|64 (read when an index is built; tuning): lanes that share one query. The default is chosen from the
 * index's mean cell population (8 lanes from 32 points per occupied cell, 1 below; DESIGN.md 4, "K18").
 */
#ifndef EG3D_NEAREST_HPP_
#define EG3D_NEAREST_HPP_
#include "../eg3d.h"
#include "host_nearest.hpp"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eg3d_cloud_index eg3d_cloud_index;

/* X_host: [n][3]; keep_host: [n] or NULL. stats may be NULL. */
int eg3d_cloud_index_build(eg3d_ctx* ctx, const float* X_host, uint64_t n, const uint8_t* keep_host, float cell,
                           eg3d_cloud_index** index, eg3d_cloud_index_stats* stats);

/* cloud: any complete cloud on ctx's device, NULL = the context's last device output; only X is read, and it is copied:
 * the index does not follow later changes of the cloud. keep_dev: [n_points] on the device, or NULL. */
int eg3d_cloud_index_build_device(eg3d_ctx* ctx, const eg3d_device_edgepoints* cloud, const uint8_t* keep_dev, float cell,
                                  eg3d_cloud_index** index, eg3d_cloud_index_stats* stats);

void eg3d_cloud_index_free(eg3d_cloud_index* index);

/* Queries resident on the device. d2_out_dev: [n_points] float, nn_out_dev: [n_points] uint32_t, either may be NULL.
 * stats (may be NULL: no thresholds) carries the thresholds in and the figures out. */
int eg3d_cloud_nearest_device(eg3d_ctx* ctx, const eg3d_device_edgepoints* cloud, const uint8_t* keep_dev,
                              eg3d_cloud_index* index, float max_dist, float* d2_out_dev, uint32_t* nn_out_dev,
                              eg3d_nearest_stats* stats);

/* the same for queries on the host, uploaded for the call; the outputs are host arrays, either may be NULL */
int eg3d_cloud_nearest_points(eg3d_ctx* ctx, const float* X_host, uint64_t n, const uint8_t* keep_host, eg3d_cloud_index* index,
                              float max_dist, float* d2_out_host, uint32_t* nn_out_host, eg3d_nearest_stats* stats);

#ifdef __cplusplus
}
#endif
#endif
