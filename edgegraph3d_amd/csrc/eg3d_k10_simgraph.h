// Host-visible declarations of K10 (eg3d_k10_simgraph.hip): the graph half of pipeline 1 of the reference, the polyline
// compatibility graph of polyline_matching_similarity_graph (eg3d_similarity_graph).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_k9_polymatch.h"

namespace eg3d {

#define K10_BLOCK 256
#define K10_NONE (~0ull)  /* node key of a polyline no point lists; directed key of an edge that is not kept */

// What the passes after the search read (all on the device):
//   pair  [n_pair]     the distinct (point, polyline) pairs as point << 32 | g, ascending: per point its cur_cams_pls
//   cp_off[n_pts + 1]  CSR of `pair` over the points of the range
//   cr_off[n_pl + 1], cr_point  close_refpoints: per global polyline index the ascending points that list it
//   weight[n_pts]      compute_refpoint_weight
//   vis   [n_pts][vis_words]  bit v of a point's row: its track lists view v (pointsVisibleFromCamN_)
//   node_g[n_nodes], node_view[n_nodes]  polyline_matches_vector, in node-id order
struct K10Graph {
  uint32_t seed_begin, n_pts, n_pl, vis_words;
  const unsigned long long* pair;
  const uint32_t* cp_off;
  const uint32_t* cr_off;
  const uint32_t* cr_point;
  const float* weight;
  const uint32_t* vis;
  const uint32_t* node_g;
  const uint32_t* node_view;
};

// (1) one wavefront per entry, twice: fill = false writes cnt[entry] = polylines with d^2 <= 100 (0 for an entry whose view
//     an earlier entry of the track names: both give the same list, which counts once); fill = true writes them, ascending,
//     as point << 32 | g behind off[entry] (the exclusive scan of cnt)
void launch_k10_close_list(hipStream_t st, bool fill, DevScene s, K9Grid g10, SeedsDev sd, uint32_t sv_base, uint32_t n_sv,
                           const uint32_t* sv_seed, uint32_t* cnt, const uint32_t* off, unsigned long long* pair);
// (2) one lane per sorted pair: cp_view / cp_pl of g, and the swapped key g << 32 | point
void launch_k10_pairs(hipStream_t st, DevScene s, const unsigned long long* pair, uint32_t n_pair, uint32_t* cp_view,
                      uint32_t* cp_pl, unsigned long long* swapped);
// (3) off[r] = lower bound of (base + r) << 32 in the ascending keys, r = 0..n_rows (n_rows + 1 lanes)
void launch_k10_row_off(hipStream_t st, const unsigned long long* keys, uint32_t n_keys, uint32_t base, uint32_t n_rows,
                        uint32_t* off);
// (4) lo[i] = low word of keys[i]
void launch_k10_low_words(hipStream_t st, const unsigned long long* keys, uint32_t n, uint32_t* lo);
// (5) one lane per point: weight, the visibility row, n_pairs[i] = m (m - 1) / 2; n_pairs[n_pts] = 0 (the scan's sentinel)
void launch_k10_points(hipStream_t st, SeedsDev sd, uint32_t seed_begin, uint32_t n_pts, const uint32_t* cp_off,
                       const uint32_t* cp_view, uint32_t vis_words, float* weight, uint32_t* vis, unsigned long long* n_pairs);
// (6) one lane per polyline: key[g] = first[g] << 32 | g, first[g] the smallest point that lists g (K10_NONE: none)
void launch_k10_node_keys(hipStream_t st, uint32_t n_pl, const uint32_t* cr_off, const uint32_t* cr_point, unsigned long long* key);
// (7) over the sorted node keys: node_of[g] = position; node_g / node_view / node_pl at it; *n_nodes (zeroed before) += nodes
void launch_k10_nodes(hipStream_t st, DevScene s, const unsigned long long* key_sorted, uint32_t n_pl, uint32_t* node_of,
                      uint32_t* node_g, uint32_t* node_view, uint32_t* node_pl, uint32_t* n_nodes);
// (8) one lane per pair instance t0 .. t0 + n of the flat sequence (point ascending, then (i, j) of its list, i < j):
//     out[k] = min node << 32 | max node. pair_off: exclusive 64-bit scan of n_pairs
void launch_k10_expand(hipStream_t st, K10Graph g, const unsigned long long* pair_off, const uint32_t* node_of,
                       unsigned long long t0, uint32_t n, unsigned long long* out);
// (9) one lane per unique edge: the weighted Jaccard compatibility; both directed keys (K10_NONE unless w > 0) with w as their
//     value; *n_kept (zeroed before) += kept edges
void launch_k10_edge_weights(hipStream_t st, K10Graph g, const unsigned long long* edges, uint32_t n_edges,
                             unsigned long long* dkey, uint32_t* dval, uint32_t* n_kept);

hipError_t k10_scan_u64(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* in, unsigned long long* out, size_t n);
// out = the distinct keys of the ascending `in`, *n_out their number
hipError_t k10_unique(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* in, unsigned long long* out,
                      uint32_t* n_out, size_t n);

}  // namespace eg3d
