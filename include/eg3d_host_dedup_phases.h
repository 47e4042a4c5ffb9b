/*
 * eg3d_host_dedup_phases.h — the 3 px de-duplication in its phases on host clouds (libeg3d_host.so): the sequential
 * definition that eg3d_dedup_claim / eg3d_dedup_keep / eg3d_dedup_merge_claims (include/eg3d_dedup_phases.h) are compared
 * with, and what a run on host arrays (distributed.HostCloudGather) uses to do the same thing.
 *
 * A claim map `first` has eg3d_host_dedup_n_cells(n_views, width, height) = n_views * ceil(width / 3) * ceil(height / 3)
 * entries [view][cell row][cell column], the caller's array, 0xFFFFFFFF = untouched (the caller fills it). The cell of an
 * observation is that of eg3d_host_filter_close_2d (one function in host/post_steps.cpp serves both). Claim the clouds of a
 * run in any order, each with its run-wide index_base, into one map or into several joined by eg3d_host_dedup_merge; keep
 * then gives, part by part, the mask eg3d_host_filter_close_2d gives on the concatenation of the clouds in index order.
 *
 * All return 0, or -1 for bad arguments: a null array, n_views <= 0, index_base + n_points not below 2^32 - 1, or a list
 * that is not an ascending range inside [0, n_obs] (obs_off carries its sentinel, as every host cloud's). A refused call
 * has written nothing.
 */
#ifndef EG3D_HOST_DEDUP_PHASES_H_
#define EG3D_HOST_DEDUP_PHASES_H_
#include "eg3d_host.h"

#ifdef __cplusplus
extern "C" {
#endif

uint64_t eg3d_host_dedup_n_cells(int n_views, int width, int height);
/* first[cell] = min(first[cell], index_base + i) for every observation of every point i that has a cell */
int eg3d_host_dedup_claim(int n_views, int width, int height, const eg3d_edgepoints* pts, uint64_t index_base,
                          uint32_t* first);
/* keep[i] = 1 when an observation of point i lies in a cell that holds index_base + i; n_kept may be NULL */
int eg3d_host_dedup_keep(int n_views, int width, int height, const eg3d_edgepoints* pts, uint64_t index_base,
                         const uint32_t* first, uint8_t* keep, uint64_t* n_kept);
/* first[c] = min(first[c], other[c]) for c < n_cells */
int eg3d_host_dedup_merge(uint32_t* first, const uint32_t* other, uint64_t n_cells);

#ifdef __cplusplus
}
#endif
#endif
