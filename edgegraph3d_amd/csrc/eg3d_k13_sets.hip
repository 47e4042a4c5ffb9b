// eg3d_k13_sets.hip — K13: polyline sets that stay on the device (include/eg3d_sets_device.h).
//
// compute_polyline_matches_from_nodes_component_ids (matching/polyline_matching/polyline_matcher.cpp:202-214) turns the
// community id of every node of the compatibility graph into one id set per (community, view): max id + 1 communities, a
// node with a negative id in none, a community nobody names an empty set, a (view, polyline) named twice once. As every
// list of this project it is built by sorting, never by appending:
//   k13_validate    1 lane / node   named = id >= 0; max id + 1 by 64-bit atomicMax; view and polyline id checked
//   (scan of `named`, eg3d_api_sets.hip)
//   k13_keys        1 lane / node   (id * V + view) << 19 | pl behind the scan                   (the key of K9's tail)
//   (rocPRIM radix sort, then the distinct keys; k0_grid_csr writes row_off / pl_ids over n_sets * V "cells")
// and the checks of a caller's uploaded sets (eg3d_upload_polyline_sets), which run before any id is used as an index:
//   k13_check_rows  1 lane / row boundary   row_off[0] == 0, row_off ascends
//   k13_check_ids   1 lane / id             id below its view's polyline count, strictly above the id before it in its row
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_pipeline.h"
#include "eg3d_k13_sets.h"

namespace eg3d {

static_assert(EG3D_K0_PL_BITS_HOST == 19, "the key of k13_keys is the key of k0_grid_csr");

__global__ void __launch_bounds__(K13_BLOCK) k13_validate(const int64_t* ids, const uint32_t* node_view, const uint32_t* node_pl,
                                                          uint32_t n, uint32_t n_views, uint32_t* named,
                                                          unsigned long long* counters) {
  const uint32_t i = blockIdx.x * K13_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int64_t id = ids[i];
  named[i] = id >= 0 ? 1u : 0u;
  if (id < 0) return;
  const unsigned long long sets = (unsigned long long)id + 1ull;
  if (sets > counters[0]) atomicMax(&counters[0], sets);  // (the plain read only saves atomics: the maximum never falls)
  uint32_t bad = 0;
  if (node_view[i] >= n_views) bad |= K13_BAD_VIEW;
  if (node_pl[i] >> EG3D_K0_PL_BITS_HOST) bad |= K13_BAD_PL;
  if (bad) atomicOr(&counters[1], (unsigned long long)bad);
}

__global__ void __launch_bounds__(K13_BLOCK) k13_keys(const int64_t* ids, const uint32_t* node_view, const uint32_t* node_pl, uint32_t n,
                                                      uint32_t n_views, const uint32_t* named, const uint32_t* pos,
                                                      unsigned long long* keys) {
  const uint32_t i = blockIdx.x * K13_BLOCK + threadIdx.x;
  if (i >= n || !named[i]) return;
  const unsigned long long row = (unsigned long long)ids[i] * n_views + node_view[i];  // (< 2^32 - 1: checked on the host)
  keys[pos[i]] = row << EG3D_K0_PL_BITS_HOST | node_pl[i];
}

__global__ void __launch_bounds__(K13_BLOCK) k13_check_rows(const uint32_t* row_off, uint32_t n_rows, uint32_t* bad) {
  const uint32_t r = blockIdx.x * K13_BLOCK + threadIdx.x;
  if (r > n_rows) return;
  if (r == n_rows) {  // (the lane behind the last row looks at the first offset)
    if (row_off[0] != 0u) atomicOr(bad, K13_SETS_BAD_START);
    return;
  }
  if (row_off[r + 1] < row_off[r]) atomicOr(bad, K13_SETS_BAD_ORDER);
}

__global__ void __launch_bounds__(K13_BLOCK) k13_check_ids(DevScene s, SetsDev sets, uint32_t n_rows, uint32_t n_ids, uint32_t* bad) {
  const uint32_t k = blockIdx.x * K13_BLOCK + threadIdx.x;
  if (k >= n_ids) return;
  const uint32_t row = find_owner(sets.row_off, n_rows, k);  // (0 .. n_rows - 1 whatever the offsets hold)
  const uint32_t view = row % sets.n_views;
  const uint32_t id = sets.pl_ids[k];
  if (id >= s.view_pl_off[view + 1] - s.view_pl_off[view]) atomicOr(bad, K13_SETS_BAD_RANGE);
  if (k > sets.row_off[row] && id <= sets.pl_ids[k - 1]) atomicOr(bad, K13_SETS_BAD_STRICT);
}

void launch_k13_validate(hipStream_t st, const int64_t* ids, const uint32_t* node_view, const uint32_t* node_pl, uint32_t n,
                         uint32_t n_views, uint32_t* named, unsigned long long* counters) {
  if (!n) return;
  hipLaunchKernelGGL(k13_validate, blocks_for(n, K13_BLOCK), dim3(K13_BLOCK), 0, st, ids, node_view, node_pl, n, n_views, named, counters);
}
void launch_k13_keys(hipStream_t st, const int64_t* ids, const uint32_t* node_view, const uint32_t* node_pl, uint32_t n,
                     uint32_t n_views, const uint32_t* named, const uint32_t* pos, unsigned long long* keys) {
  if (!n) return;
  hipLaunchKernelGGL(k13_keys, blocks_for(n, K13_BLOCK), dim3(K13_BLOCK), 0, st, ids, node_view, node_pl, n, n_views, named, pos, keys);
}
void launch_k13_check_sets(hipStream_t st, DevScene s, SetsDev sets, uint32_t n_rows, uint32_t n_ids, uint32_t* bad) {
  hipLaunchKernelGGL(k13_check_rows, blocks_for((uint64_t)n_rows + 1, K13_BLOCK), dim3(K13_BLOCK), 0, st, sets.row_off, n_rows, bad);
  if (n_ids && n_rows)
    hipLaunchKernelGGL(k13_check_ids, blocks_for(n_ids, K13_BLOCK), dim3(K13_BLOCK), 0, st, s, sets, n_rows, n_ids, bad);
}

}  // namespace eg3d
