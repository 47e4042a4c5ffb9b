// eg3d_k10_simgraph.hip — K10: the graph half of pipeline 1 of the reference, polyline_matching_similarity_graph
// (matching/polyline_matching/polyline_matcher.cpp:222-327), on the device.
//
// The reference, per reference point in ascending order: the polylines within 10 px of the point's observation in every
// view of its track (the search of K9); the distinct (view, polyline) pairs found are a clique of a graph whose nodes are
// numbered by first appearance, and the point is appended to close_refpoints of each. A point weighs (views with a close
// polyline) / (float)(pairs); an edge ((v1, p1), (v2, p2)) weighs sum(weight over A and B) / sum(weight over A or B), A the
// points close to p1 on v1 whose track lists v2, B the points close to p2 on v2 whose track lists v1, each sum a float that
// adds in ascending point order; edges with w > 0 make the weighted adjacency.
//
// Nothing below depends on the order in which lanes arrive. A node's id grows with (first point that lists it, (view,
// polyline)), and (view, polyline) ascending is the global polyline index g ascending, so the id is the rank of
// first[g] << 32 | g (K9's argument); lists are made by sorting 64-bit keys, never by appending:
//   k10_close_list<fill>  1 WAVE / entry          the search of k9_close_polylines in list form: count, scan, fill
//   k10_pairs             1 lane / (point, g)     close_polylines' columns; the key g << 32 | point of close_refpoints
//   k10_row_off           1 lane / row            CSR offsets of a sorted key array by binary search
//   k10_points            1 lane / point          weight, visibility bits, m (m - 1) / 2
//   k10_node_keys, k10_nodes   1 lane / polyline  first[g] << 32 | g; after the sort: node ids
//   k10_expand            1 lane / pair instance  the cliques, a chunk of the flat instance sequence at a time
//   k10_edge_weights      1 lane / unique edge    the two-list walk; both directed keys of a kept edge
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "eg3d_dev_pipeline.h"
#include "eg3d_dev_coopgn.h"
#include "eg3d_k10_simgraph.h"

namespace eg3d {

// One wavefront per (reference point, track entry): k9_close_polylines' search — lanes 0..8 own the cells of the (shrunk)
// 3x3 window of the 10 px map and k-way-merge their ascending id lists, 64 candidates at a time; the segments of a batch
// are one flat sequence and the closest segment of a candidate is the 64-bit minimum (distance bits : segment) in its LDS
// slot. Candidates leave the merge ascending, so the close ones of a batch are written in lane order behind those of the
// batches before: the list is ascending without a sort.
template <bool FILL>
__global__ void __launch_bounds__(K10_BLOCK) k10_close_list(DevScene s, K9Grid g10, SeedsDev sd, uint32_t sv_base, uint32_t n_sv,
                                                            const uint32_t* sv_seed, uint32_t* cnt, const uint32_t* off,
                                                            unsigned long long* pair) {
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  if (wave >= n_sv) return;
  const uint32_t sv = wave;
  const uint32_t seed = sv_seed[sv];
  const uint32_t t0 = sd.trk_off[seed], k = sd.trk_off[seed + 1] - t0;
  const int32_t view = sd.trk_view[sv_base + sv];
  bool again = false;  // an earlier entry of the track names the view: the same observation, the same list, counted once
  for (uint32_t f = t0 + lane; f < sv_base + sv; f += 64) again = again || sd.trk_view[f] == view;
  if (__ballot(again)) {
    if (!FILL && lane == 0) cnt[sv] = 0;
    return;
  }
  float px, py;
  seed_obs_in_view(sd, t0, k, view, px, py);
  const CellWindow w = cell_window(10.0f, s.width, s.height, g10.w, g10.h, px, py);
  uint32_t a = 0, b = 0;
  if (w.c1 >= w.c0) {
    const int ncols = w.c1 - w.c0 + 1, nrows = w.r1 - w.r0 + 1;
    if ((int)lane < ncols * nrows) {
      const int r = w.r0 + (int)lane / ncols, c = w.c0 + (int)lane % ncols;
      const size_t cell = (size_t)view * (size_t)(g10.w * g10.h) + (size_t)r * g10.w + c;
      a = g10.off[cell];
      b = g10.off[cell + 1];
    }
  }
  __shared__ unsigned long long k10_best[K10_BLOCK / 64][64];
  unsigned long long* const slot = k10_best[threadIdx.x >> 6];
  const uint32_t gview = s.view_pl_off[view];
  const uint32_t out0 = FILL ? off[sv] : 0u;
  uint32_t n_close = 0;
  for (;;) {
    uint32_t my_id = 0xffffffffu, nb = 0;
    while (nb < 64) {  // phase A: one wave minimum of the list heads per candidate
      const uint32_t head = a < b ? g10.ids[a] : 0xffffffffu;
      const uint32_t m = wave_min_u32_dpp(head);
      if (m == 0xffffffffu) break;
      if (head == m) a++;
      if (lane == nb) my_id = m;
      nb++;
    }
    if (nb == 0) break;
    uint32_t my_a = 0, my_n = 0;
    if (lane < nb) {
      const uint32_t v0 = s.pl_vtx_off[gview + my_id], v1 = s.pl_vtx_off[gview + my_id + 1];
      my_a = v0;
      my_n = v1 - v0;
    }
    const uint32_t my_ns = my_n >= 2u ? my_n - 1u : 0u;
    const uint32_t incl = (uint32_t)wave_incl_scan((int)my_ns);
    const uint32_t total = (uint32_t)lane_bcast((int)incl, 63);
    slot[lane] = ~0ull;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t base = 0; base < total; base += 64) {  // phase B: the batch's segments as one flat sequence
      const uint32_t f = base + lane;
      uint32_t pos = 0;  // owner of flat segment f: the first lane whose inclusive count exceeds f
#pragma unroll
      for (uint32_t step = 32; step; step >>= 1) {
        const uint32_t v = (uint32_t)__shfl((int)incl, (int)(pos + step - 1), 64);
        if (v <= f) pos += step;
      }
      const uint32_t o_incl = (uint32_t)__shfl((int)incl, (int)pos, 64);
      const uint32_t o_ns = (uint32_t)__shfl((int)my_ns, (int)pos, 64);
      const uint32_t o_a = (uint32_t)__shfl((int)my_a, (int)pos, 64);
      if (f < total) {
        const uint32_t j = f - (o_incl - o_ns);
        const f2 v0 = s.vtx[o_a + j], v1 = s.vtx[o_a + j + 1];
        float qx, qy;
        const float d = seg_closest(px, py, v0.x, v0.y, v1.x, v1.y, qx, qy);
        if (d < __builtin_huge_valf())
          atomicMin(&slot[pos], ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)j);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const unsigned long long key = slot[lane];
    const float dmin = __uint_as_float((uint32_t)(key >> 32));
    const bool close = lane < nb && key != ~0ull && dmin <= 100.0f;  // (no finite distance: never a result, as in K1)
    const unsigned long long mc = __ballot(close);
    if (FILL && close)
      pair[out0 + n_close + (uint32_t)__popcll(mc & ((1ull << lane) - 1ull))] =
          ((unsigned long long)seed << 32) | (unsigned long long)(gview + my_id);
    n_close += (uint32_t)__popcll(mc);
    __builtin_amdgcn_wave_barrier();
    if (nb < 64) break;
  }
  if (!FILL && lane == 0) cnt[sv] = n_close;
}

// view of global polyline g: the last v with view_pl_off[v] <= g (as K0)
__device__ __forceinline__ uint32_t k10_view_of(const DevScene& s, uint32_t g) {
  uint32_t lo = 0, hi = (uint32_t)s.n_views;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (s.view_pl_off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(K10_BLOCK) k10_pairs(DevScene s, const unsigned long long* pair, uint32_t n_pair,
                                                       uint32_t* cp_view, uint32_t* cp_pl, unsigned long long* swapped) {
  const uint32_t i = blockIdx.x * K10_BLOCK + threadIdx.x;
  if (i >= n_pair) return;
  const unsigned long long key = pair[i];
  const uint32_t g = (uint32_t)key, v = k10_view_of(s, g);
  cp_view[i] = v;
  cp_pl[i] = g - s.view_pl_off[v];
  swapped[i] = ((unsigned long long)g << 32) | (key >> 32);
}

__global__ void __launch_bounds__(K10_BLOCK) k10_row_off(const unsigned long long* keys, uint32_t n_keys, uint32_t base,
                                                         uint32_t n_rows, uint32_t* off) {
  const uint32_t r = blockIdx.x * K10_BLOCK + threadIdx.x;
  if (r > n_rows) return;
  const unsigned long long want = ((unsigned long long)base + r) << 32;
  uint32_t lo = 0, hi = n_keys;  // first position whose key is >= want
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  off[r] = lo;
}

__global__ void __launch_bounds__(K10_BLOCK) k10_low_words(const unsigned long long* keys, uint32_t n, uint32_t* lo) {
  const uint32_t i = blockIdx.x * K10_BLOCK + threadIdx.x;
  if (i < n) lo[i] = (uint32_t)keys[i];
}

// compute_refpoint_weight (polyline_matcher.cpp:191-200): an int divided by a float. The list of a point ascends in g, so
// its views ascend and the views with a close polyline are the changes of view along it.
__global__ void __launch_bounds__(K10_BLOCK) k10_points(SeedsDev sd, uint32_t seed_begin, uint32_t n_pts, const uint32_t* cp_off,
                                                        const uint32_t* cp_view, uint32_t vis_words, float* weight,
                                                        uint32_t* vis, unsigned long long* n_pairs) {
  const uint32_t i = blockIdx.x * K10_BLOCK + threadIdx.x;
  if (i > n_pts) return;
  if (i == n_pts) {
    n_pairs[i] = 0;
    return;
  }
  const uint32_t p0 = cp_off[i], m = cp_off[i + 1] - p0;
  int non_empty = 0;
  for (uint32_t j = 0; j < m; j++) non_empty += (j == 0 || cp_view[p0 + j] != cp_view[p0 + j - 1]) ? 1 : 0;
  weight[i] = m ? (float)non_empty / (float)(int)m : 0.0f;
  n_pairs[i] = (unsigned long long)m * (unsigned long long)(m ? m - 1 : 0) / 2ull;
  uint32_t* const row = vis + (size_t)i * vis_words;
  for (uint32_t wd = 0; wd < vis_words; wd++) row[wd] = 0;
  const uint32_t t0 = sd.trk_off[seed_begin + i], t1 = sd.trk_off[seed_begin + i + 1];
  for (uint32_t e = t0; e < t1; e++) {  // (the lane owns the row: plain read-modify-write)
    const uint32_t v = (uint32_t)sd.trk_view[e];
    row[v >> 5] |= 1u << (v & 31u);
  }
}

__global__ void __launch_bounds__(K10_BLOCK) k10_node_keys(uint32_t n_pl, const uint32_t* cr_off, const uint32_t* cr_point,
                                                           unsigned long long* key) {
  const uint32_t g = blockIdx.x * K10_BLOCK + threadIdx.x;
  if (g >= n_pl) return;
  const uint32_t a = cr_off[g];
  key[g] = cr_off[g + 1] > a ? ((unsigned long long)cr_point[a] << 32) | (unsigned long long)g : K10_NONE;
}

__global__ void __launch_bounds__(K10_BLOCK) k10_nodes(DevScene s, const unsigned long long* key_sorted, uint32_t n_pl,
                                                       uint32_t* node_of, uint32_t* node_g, uint32_t* node_view,
                                                       uint32_t* node_pl, uint32_t* n_nodes) {
  const uint32_t j = blockIdx.x * K10_BLOCK + threadIdx.x;
  const bool node = j < n_pl && key_sorted[j] != K10_NONE;
  if (node) {
    const uint32_t g = (uint32_t)key_sorted[j], v = k10_view_of(s, g);
    node_of[g] = j;
    node_g[j] = g;
    node_view[j] = v;
    node_pl[j] = g - s.view_pl_off[v];
  }
  const uint32_t n = (uint32_t)__popcll(__ballot(node));
  if ((threadIdx.x & 63u) == 0 && n) atomicAdd(n_nodes, n);
}

// Pair instance t of the flat sequence belongs to the last point r with pair_off[r] <= t (points without pairs share their
// successor's offset and are passed over); q = t - pair_off[r] is the position of (i, j), i < j, among the m (m - 1) / 2
// pairs of its list in row-major order: row i starts at i (2 m - i - 1) / 2.
__global__ void __launch_bounds__(K10_BLOCK) k10_expand(K10Graph g, const unsigned long long* pair_off, const uint32_t* node_of,
                                                        unsigned long long t0, uint32_t n, unsigned long long* out) {
  const uint32_t k = blockIdx.x * K10_BLOCK + threadIdx.x;
  if (k >= n) return;
  const unsigned long long t = t0 + k;
  uint32_t lo = 0, hi = g.n_pts;  // pair_off[lo] <= t < pair_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (pair_off[mid] <= t) lo = mid; else hi = mid;
  }
  const uint32_t p0 = g.cp_off[lo], m = g.cp_off[lo + 1] - p0;
  const unsigned long long q = t - pair_off[lo];
  uint32_t il = 0, ih = m - 1;  // row(il) <= q < row(ih)
  while (ih - il > 1) {
    const uint32_t mid = il + ((ih - il) >> 1);
    if ((unsigned long long)mid * (2ull * m - mid - 1ull) / 2ull <= q) il = mid; else ih = mid;
  }
  const uint32_t j = il + 1u + (uint32_t)(q - (unsigned long long)il * (2ull * m - il - 1ull) / 2ull);
  const uint32_t na = node_of[(uint32_t)g.pair[p0 + il]], nb = node_of[(uint32_t)g.pair[p0 + j]];
  out[k] = na < nb ? ((unsigned long long)na << 32) | nb : ((unsigned long long)nb << 32) | na;
}

__device__ __forceinline__ bool k10_lists(const K10Graph& g, uint32_t point, uint32_t view) {
  return (g.vis[(size_t)(point - g.seed_begin) * g.vis_words + (view >> 5)] >> (view & 31u)) & 1u;
}

// compute_compatibility (polyline_matcher.cpp:171-189) on the two ascending rows of close_refpoints, filtered as
// close_refpoints_divided_by_visibility is (:297-307): one walk visits the union in ascending point order, and the two
// float sums add in that order, as the reference's loops over set_intersection and set_union do.
__global__ void __launch_bounds__(K10_BLOCK) k10_edge_weights(K10Graph g, const unsigned long long* edges, uint32_t n_edges,
                                                              unsigned long long* dkey, uint32_t* dval, uint32_t* n_kept) {
  const uint32_t e = blockIdx.x * K10_BLOCK + threadIdx.x;
  bool kept = false;
  if (e < n_edges) {
    const uint32_t n1 = (uint32_t)(edges[e] >> 32), n2 = (uint32_t)edges[e];
    const uint32_t g1 = g.node_g[n1], g2 = g.node_g[n2], v1 = g.node_view[n1], v2 = g.node_view[n2];
    uint32_t ia = g.cr_off[g1], ib = g.cr_off[g2];
    const uint32_t ea = g.cr_off[g1 + 1], eb = g.cr_off[g2 + 1];
    float inter = 0.0f, uni = 0.0f;
    for (;;) {
      while (ia < ea && !k10_lists(g, g.cr_point[ia], v2)) ia++;
      while (ib < eb && !k10_lists(g, g.cr_point[ib], v1)) ib++;
      if (ia == ea && ib == eb) break;
      const uint32_t ra = ia < ea ? g.cr_point[ia] : 0xffffffffu, rb = ib < eb ? g.cr_point[ib] : 0xffffffffu;
      const uint32_t r = ra < rb ? ra : rb;
      const float wr = g.weight[r - g.seed_begin];
      uni += wr;
      if (ra == rb) inter += wr;
      if (ra == r) ia++;
      if (rb == r) ib++;
    }
    const float w = inter == 0.0f ? 0.0f : inter / uni;
    kept = w > 0.0f;
    dkey[2 * (size_t)e] = kept ? ((unsigned long long)n1 << 32) | n2 : K10_NONE;
    dkey[2 * (size_t)e + 1] = kept ? ((unsigned long long)n2 << 32) | n1 : K10_NONE;
    dval[2 * (size_t)e] = dval[2 * (size_t)e + 1] = __float_as_uint(w);
  }
  const uint32_t n = (uint32_t)__popcll(__ballot(kept));
  if ((threadIdx.x & 63u) == 0 && n) atomicAdd(n_kept, n);
}

// ------------------------------------------------------------ launch wrappers --
void launch_k10_close_list(hipStream_t st, bool fill, DevScene s, K9Grid g10, SeedsDev sd, uint32_t sv_base, uint32_t n_sv,
                           const uint32_t* sv_seed, uint32_t* cnt, const uint32_t* off, unsigned long long* pair) {
  if (!n_sv) return;
  const dim3 grid = blocks_for((uint64_t)n_sv * 64, K10_BLOCK);
  if (fill)
    hipLaunchKernelGGL(k10_close_list<true>, grid, dim3(K10_BLOCK), 0, st, s, g10, sd, sv_base, n_sv, sv_seed, cnt, off, pair);
  else
    hipLaunchKernelGGL(k10_close_list<false>, grid, dim3(K10_BLOCK), 0, st, s, g10, sd, sv_base, n_sv, sv_seed, cnt, off, pair);
}
void launch_k10_pairs(hipStream_t st, DevScene s, const unsigned long long* pair, uint32_t n_pair, uint32_t* cp_view,
                      uint32_t* cp_pl, unsigned long long* swapped) {
  if (!n_pair) return;
  hipLaunchKernelGGL(k10_pairs, blocks_for(n_pair, K10_BLOCK), dim3(K10_BLOCK), 0, st, s, pair, n_pair, cp_view, cp_pl, swapped);
}
void launch_k10_row_off(hipStream_t st, const unsigned long long* keys, uint32_t n_keys, uint32_t base, uint32_t n_rows,
                        uint32_t* off) {
  hipLaunchKernelGGL(k10_row_off, blocks_for((uint64_t)n_rows + 1, K10_BLOCK), dim3(K10_BLOCK), 0, st, keys, n_keys, base, n_rows, off);
}
void launch_k10_low_words(hipStream_t st, const unsigned long long* keys, uint32_t n, uint32_t* lo) {
  if (!n) return;
  hipLaunchKernelGGL(k10_low_words, blocks_for(n, K10_BLOCK), dim3(K10_BLOCK), 0, st, keys, n, lo);
}
void launch_k10_points(hipStream_t st, SeedsDev sd, uint32_t seed_begin, uint32_t n_pts, const uint32_t* cp_off,
                       const uint32_t* cp_view, uint32_t vis_words, float* weight, uint32_t* vis, unsigned long long* n_pairs) {
  hipLaunchKernelGGL(k10_points, blocks_for((uint64_t)n_pts + 1, K10_BLOCK), dim3(K10_BLOCK), 0, st, sd, seed_begin, n_pts, cp_off,
                     cp_view, vis_words, weight, vis, n_pairs);
}
void launch_k10_node_keys(hipStream_t st, uint32_t n_pl, const uint32_t* cr_off, const uint32_t* cr_point, unsigned long long* key) {
  if (!n_pl) return;
  hipLaunchKernelGGL(k10_node_keys, blocks_for(n_pl, K10_BLOCK), dim3(K10_BLOCK), 0, st, n_pl, cr_off, cr_point, key);
}
void launch_k10_nodes(hipStream_t st, DevScene s, const unsigned long long* key_sorted, uint32_t n_pl, uint32_t* node_of,
                      uint32_t* node_g, uint32_t* node_view, uint32_t* node_pl, uint32_t* n_nodes) {
  if (!n_pl) return;
  hipLaunchKernelGGL(k10_nodes, blocks_for(n_pl, K10_BLOCK), dim3(K10_BLOCK), 0, st, s, key_sorted, n_pl, node_of, node_g, node_view,
                     node_pl, n_nodes);
}
void launch_k10_expand(hipStream_t st, K10Graph g, const unsigned long long* pair_off, const uint32_t* node_of,
                       unsigned long long t0, uint32_t n, unsigned long long* out) {
  if (!n) return;
  hipLaunchKernelGGL(k10_expand, blocks_for(n, K10_BLOCK), dim3(K10_BLOCK), 0, st, g, pair_off, node_of, t0, n, out);
}
void launch_k10_edge_weights(hipStream_t st, K10Graph g, const unsigned long long* edges, uint32_t n_edges,
                             unsigned long long* dkey, uint32_t* dval, uint32_t* n_kept) {
  if (!n_edges) return;
  hipLaunchKernelGGL(k10_edge_weights, blocks_for(n_edges, K10_BLOCK), dim3(K10_BLOCK), 0, st, g, edges, n_edges, dkey, dval, n_kept);
}

hipError_t k10_scan_u64(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* in, unsigned long long* out, size_t n) {
  return rocprim::exclusive_scan(tmp, tmp_bytes, in, out, 0ull, n, rocprim::plus<unsigned long long>(), st);
}
hipError_t k10_unique(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* in, unsigned long long* out,
                      uint32_t* n_out, size_t n) {
  return rocprim::unique(tmp, tmp_bytes, in, out, n_out, n, rocprim::equal_to<unsigned long long>(), st);
}

}  // namespace eg3d
