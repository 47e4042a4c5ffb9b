// Host-visible declarations of K18 (eg3d_k18_nearest.hip): the uniform-grid index over a point set and the nearest
// distances of a second point set against it (include/eg3d/nearest.hpp; the arithmetic: eg3d_nearest_core.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_nearest_core.h"

namespace eg3d {

#define K18_BLOCK 256
#define K18_MAX_BLOCKS 4096 /* grid-stride kernels: 16 384 wavefronts at most, each ends in a handful of atomics */

// the counters of a build (64-bit words): what the reduction leaves ...
enum { K18B_DROPPED, K18B_NONFINITE, K18B_MIN, K18B_MAX = K18B_MIN + 3, K18B_MAXCELL = K18B_MAX + 3, K18B_COUNT };
// ... and of a query: the figures of include/eg3d/host_nearest.hpp
enum { K18Q_DROPPED, K18Q_NONFINITE, K18Q_WITHIN, K18Q_SUM, K18Q_BELOW, K18Q_MIN = K18Q_BELOW + nearest::kMaxThresholds, K18Q_MAX,
       K18Q_MEDIAN, K18Q_COUNT };

struct K18Thresholds {
  float t2[nearest::kMaxThresholds];  // t_k * t_k in FP32; 0 for a threshold that is not given
};

// the counters at their neutral values (min: all ones, the others 0)
void launch_k18_init(hipStream_t st, unsigned long long* ctr, bool query);
// (1) the ordered minimum and maximum of the points to index, the points keep drops, the kept non-finite ones
void launch_k18_minmax(hipStream_t st, const float* X, uint64_t n, const uint8_t* keep, unsigned long long* ctr);
// (2) per point its cell key (kUnindexed when it is not indexed) and its position
void launch_k18_keys(hipStream_t st, nearest::Grid g, const float* X, uint64_t n, const uint8_t* keep, unsigned long long* key,
                     uint32_t* val);
// (3) over the sorted pairs: the key-ordered copy of the points, and head[k] = 1 where a cell starts (head[n_indexed] = 0)
void launch_k18_gather(hipStream_t st, const float* X, const unsigned long long* key_sorted, const uint32_t* val_sorted,
                       uint64_t n_indexed, nearest::Pt* pts, uint32_t* head);
// (4) rank = exclusive scan of head over n_indexed + 1 entries: the occupied cells' keys and starts, cell_start[n_cells] = n_indexed
void launch_k18_cells(hipStream_t st, const unsigned long long* key_sorted, const uint32_t* head, const uint32_t* rank,
                      uint64_t n_indexed, unsigned long long* cell_key, uint32_t* cell_start);
// (5) the largest cell population -> ctr[K18B_MAXCELL]
void launch_k18_max_cell(hipStream_t st, const uint32_t* cell_start, uint32_t n_cells, unsigned long long* ctr);
// The query: `group` (1, 8 or 64) lanes share a query. d2_out is never null; nn_out may be.
void launch_k18_query(hipStream_t st, int group, nearest::Grid g, const float* X, uint64_t n, const uint8_t* keep, float max_dist,
                      K18Thresholds t, float* d2_out, uint32_t* nn_out, unsigned long long* ctr);
// ctr[K18Q_MEDIAN] = the element of rank (n_within - 1) / 2 of the ascending d2 bits, +inf for an empty within set
void launch_k18_median(hipStream_t st, const uint32_t* d2_sorted, unsigned long long* ctr);
// rocPRIM behind a plain signature: the d2 bits in unsigned order. tmp == nullptr: the size query.
hipError_t k18_sort_bits(hipStream_t st, void* tmp, size_t& tmp_bytes, const uint32_t* in, uint32_t* out, size_t n);

}  // namespace eg3d
