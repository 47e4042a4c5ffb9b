// Host-visible declarations of K8m (eg3d_k8m_merge.hip): the accumulator of the PLGMatchesManager replay takes the GRAPH of
// the run that follows (eg3d_replay_merge_graph, include/eg3d_replay_merge.h). The lookup of the state's table, the append of
// the new nodes, the heads against the persistent polyline keys and everything behind the state are K8a's and K8's
// kernels (eg3d_k8a_accumulate.h, eg3d_k8_replay.h), launched unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_k8a_accumulate.h"

namespace eg3d {

// what the checks OR into their flag word; K8M_FLAG_HOSTONLY is the only one that is not an argument error
enum : uint32_t { K8M_FLAG_BAD_ENDPOINT = 1u /* pl_start / pl_end >= n_nodes */, K8M_FLAG_BAD_POINT = 2u /* node_point >= later_points */,
                  K8M_FLAG_BAD_OFFSETS = 4u /* iv_off: not from 0, not ascending, or a row longer than its polyline has segments */,
                  K8M_FLAG_BAD_SEG = 8u /* a start or end segment outside its scene polyline */,
                  K8M_FLAG_HOSTONLY = 16u /* a NaN coordinate, or x or y == -1, in node_X */,
                  K8M_FLAG_SEG_ORDER = 32u /* start segments of a scene polyline not strictly ascending */,
                  K8M_FLAG_DUP_NODE = 64u /* two nodes with equal canonical coordinates */,
                  K8M_FLAG_DUP_PL = 128u /* two polylines on one unordered node pair */ };

// The arrays of `later` that the merge reads (eg3d_device_graph3d without the connections).
struct K8mGraph {
  uint64_t n_nodes, n_pl;
  const float* node_X;
  const unsigned long long* node_point;
  const uint32_t* pl_start;
  const uint32_t* pl_end;
  const unsigned long long* iv_off;  // [n_scene_pl + 1]
  const uint32_t* iv_start_seg;
  const float* iv_start_xy;
  const uint32_t* iv_end_seg;
  const float* iv_end_xy;
};

// (1) one lane per node, per polyline and per scene polyline: everything that has to hold before any value of `later` is used
//     as an index. *flags zeroed before. With no K8M_FLAG_BAD_OFFSETS, iv_off[n_scene_pl] <= the scene's vertices.
void launch_k8m_check(hipStream_t st, K8mGraph b, DevScene s, uint32_t n_scene_pl, uint64_t later_points, uint32_t* flags);
// (2) after (1) passed, one lane per interval (n_iv = iv_off[n_scene_pl]): segments inside the row's scene polyline, start
//     segments strictly ascending within a row
void launch_k8m_iv_check(hipStream_t st, K8mGraph b, DevScene s, uint32_t n_scene_pl, uint64_t n_iv, uint32_t* flags);
// (3) one lane per node: into the scratch table `t` (filled with K8_EMPTY; more slots than nodes), compared through
//     later's own node_X: a node that meets its coordinates raises K8M_FLAG_DUP_NODE. Also what K8a's node kernels want per
//     "first point": every[b] = 1 and last_of[b] = node_point[b] (below 2^32: checked by (1)).
void launch_k8m_node_group(hipStream_t st, K8mGraph b, K8aTable t, uint32_t* every, uint32_t* last_of, uint32_t* flags);
// (4) per polyline j the key min(na, nb) << 32 | max(na, nb) of its endpoints mapped through node_id (nullptr: as they are),
//     with the value j
void launch_k8m_pl_keys(hipStream_t st, K8mGraph b, const uint32_t* node_id, unsigned long long* key, uint32_t* val);
// (5) over sorted keys: two equal neighbours raise K8M_FLAG_DUP_PL
void launch_k8m_pl_dups(hipStream_t st, const unsigned long long* key_sorted, uint64_t n, uint32_t* flags);
// (6) pl_id = exclusive scan of creates (K8a's k8a_pl_heads over the stably sorted mapped keys): polyline n_pl + pl_id[j] of
//     the state gets the mapped endpoints of later's polyline j, in its orientation, and its key
void launch_k8m_pl_write(hipStream_t st, K8mGraph b, const uint32_t* node_id, const uint32_t* creates, const uint32_t* pl_id,
                         uint64_t n_pl, uint32_t* pl_start, uint32_t* pl_end, unsigned long long* pl_key);
// (7) one lane per interval: a cell of the claim map that nobody holds is claimed with `id` and takes later's record; *n_iv
//     counts them. (A row names a cell once — (2) — so no two lanes meet.)
void launch_k8m_iv(hipStream_t st, K8mGraph b, DevScene s, uint32_t n_scene_pl, uint64_t n_iv, unsigned long long id,
                   unsigned long long* map, K8aRecords r, unsigned long long* n_iv_state);

}  // namespace eg3d
