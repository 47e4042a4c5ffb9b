// eg3d_k9_polymatch.hip — K9: pipeline 2 of the reference, polyline_matching_closeness_to_refpoints
// (matching/polyline_matching/polyline_matcher.cpp:75-168, called from pipelines.cpp:113-158), on the device.
//
// The reference, per reference point in ascending order: the polylines within 10 px of the point's observation in every
// view of its track (PolyLine2DMapSearch on a 10 px map, polyLine_2d_map_search.cpp:46-77,122-137); the point is accepted
// when no view answers with more than one polyline, the distinct (view, polyline) pairs number at least 0.7 of the track
// and at least two, and the largest distance is within a factor of three of the smallest; an accepted point makes a clique
// over its pairs in a graph whose nodes are numbered by first appearance; the result is the graph's components, listed by
// their smallest node id (graph_adjacency_set_undirected_no_type.cpp:44-69), each as one ascending id set per view.
//
// Only the order of the components depends on the order of the points, and it does so through one number: a node's id
// grows with (first accepting point, (view, polyline)), and (view, polyline) ascending is the global polyline index g =
// view_pl_off[view] + pl ascending. So a component's smallest node id is the minimum over its nodes of first[g] << 32 | g,
// and the passes below do not depend on the order in which lanes arrive:
//   k9_prep             1 lane / seed          entry -> seed, view ids checked before anything else reads them
//   k9_close_polylines  1 WAVE / entry         the search, shaped like k1_seed_candidates (10 px map, d^2 <= 100 only)
//   k9_refpoint_rule    1 lane / seed          the rule; 64-bit atomicMin of the point id per node; lock-free union-find
//   k9_flatten          1 lane / polyline      root of every node, 64-bit atomicMin of the component key at the root
//   k9_rank             1 lane / sorted key    component rank                         (rocPRIM radix sort before it)
//   k9_node_keys        1 lane / polyline      (rank * V + view) << 19 | pl: sorted, k0_grid_csr writes row_off / pl_ids
//   k9_compact          1 lane / seed          the accepted ids behind an exclusive scan of the flags
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_pipeline.h"
#include "eg3d_dev_coopgn.h"
#include "eg3d_k9_polymatch.h"

namespace eg3d {

__global__ void __launch_bounds__(K9_BLOCK) k9_prep(SeedsDev sd, int32_t n_views, uint32_t seed_begin, uint32_t n_seeds,
                                                    uint32_t sv_base, uint32_t* sv_seed, uint32_t* flags) {
  const uint32_t i = blockIdx.x * K9_BLOCK + threadIdx.x;
  if (i >= n_seeds) return;
  const uint32_t seed = seed_begin + i;
  const uint32_t t0 = sd.trk_off[seed], t1 = sd.trk_off[seed + 1];
  bool bad = false;
  for (uint32_t e = t0; e < t1; e++) {
    sv_seed[e - sv_base] = seed;
    const int32_t v = sd.trk_view[e];
    bad = bad || v < 0 || v >= n_views;
  }
  if (bad) atomicOr(flags, K9_FLAG_BAD_VIEW);
}

// One wavefront per (reference point, track entry). Lanes 0..8 each own one cell of the (shrunk) 3x3 window of the 10 px
// map and k-way-merge the ascending id lists, 64 candidates at a time; the segments of a batch are scanned as one flat
// sequence and the first closest segment of every candidate is the 64-bit minimum (distance bits : segment) in its LDS
// slot — k1_seed_candidates' scheme (see there for why the bit patterns order like the distances). What leaves is the
// number of polylines with d^2 <= 100, and the id and sqrt(d^2) of the first: the rule reads them where the number is 1.
__global__ void __launch_bounds__(K9_BLOCK) k9_close_polylines(DevScene s, K9Grid g10, SeedsDev sd, uint32_t sv_base,
                                                               uint32_t n_sv, const uint32_t* sv_seed, K9Entries out) {
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  if (wave >= n_sv) return;
  const uint32_t sv = wave;
  const uint32_t seed = sv_seed[sv];
  const uint32_t t0 = sd.trk_off[seed], k = sd.trk_off[seed + 1] - t0;
  const int32_t view = sd.trk_view[sv_base + sv];
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
  __shared__ unsigned long long k9_best[K9_BLOCK / 64][64];
  unsigned long long* const slot = k9_best[threadIdx.x >> 6];
  const uint32_t gview = s.view_pl_off[view];
  uint32_t n_close = 0, first_pl = 0;
  float first_d2 = 0.f;
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
    if (mc) {
      if (!n_close) {
        const int src = __ffsll((long long)mc) - 1;
        first_pl = lane_bcast(my_id, src);
        first_d2 = lane_bcast(dmin, src);
      }
      n_close += (uint32_t)__popcll(mc);
    }
    __builtin_amdgcn_wave_barrier();
    if (nb < 64) break;
  }
  if (lane == 0) {
    out.cnt[sv] = n_close;
    out.pl[sv] = first_pl;
    out.dist[sv] = __builtin_sqrtf(first_d2);
  }
}

__global__ void __launch_bounds__(K9_BLOCK) k9_init(uint32_t n_pl, K9Graph g) {
  const uint32_t i = blockIdx.x * K9_BLOCK + threadIdx.x;
  if (i >= n_pl) return;
  g.parent[i] = i;
  g.first[i] = K9_NONE;
  g.ckey[i] = K9_NONE;
}

// Lock-free union-find: a root is only ever hooked under a SMALLER index (atomicCAS from "still a root"), so parent[g] <= g
// holds throughout, there are no cycles, and the partition is the same whatever the order of the unions.
__device__ __forceinline__ uint32_t k9_find(const uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}
__device__ __forceinline__ void k9_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = k9_find(parent, a);
    b = k9_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(parent + a, a, b) == a) return;
  }
}

// polyline_matcher.cpp:106-148, the comparisons in the reference's types: the share of the track in double, the two ratio
// tests in float. max_dist starts at numeric_limits<float>::min(), the smallest positive NORMAL float: a point whose
// distances are all 0 is rejected (0 < FLT_MIN / 3).
__global__ void __launch_bounds__(K9_BLOCK) k9_refpoint_rule(DevScene s, SeedsDev sd, uint32_t seed_begin, uint32_t n_seeds,
                                                             uint32_t sv_base, K9Entries in, uint32_t* accept, K9Graph g) {
  const uint32_t i = blockIdx.x * K9_BLOCK + threadIdx.x;
  if (i > n_seeds) return;
  if (i == n_seeds) {
    accept[i] = 0;
    return;
  }
  const uint32_t seed = seed_begin + i;
  const uint32_t t0 = sd.trk_off[seed], t1 = sd.trk_off[seed + 1], n = t1 - t0;
  uint32_t maxpl = 0;
  for (uint32_t e = t0; e < t1; e++) {
    const uint32_t c = in.cnt[e - sv_base];
    maxpl = c > maxpl ? c : maxpl;
  }
  bool ok = maxpl == 1;
  if (ok) {
    float min_dist = 3.40282347e+38f, max_dist = 1.17549435e-38f;
    uint32_t n_pairs = 0;  // |S|: distinct (view, polyline); a track may list a view twice
    for (uint32_t e = t0; e < t1; e++) {
      if (!in.cnt[e - sv_base]) continue;
      const float d = in.dist[e - sv_base];
      min_dist = min_dist <= d ? min_dist : d;
      max_dist = max_dist >= d ? max_dist : d;
      bool seen = false;
      for (uint32_t f = t0; f < e && !seen; f++)
        seen = in.cnt[f - sv_base] && sd.trk_view[f] == sd.trk_view[e] && in.pl[f - sv_base] == in.pl[e - sv_base];
      n_pairs += seen ? 0u : 1u;
    }
    ok = !((double)n_pairs < (double)n * 0.7) && !(min_dist < max_dist / 3.0f) && !(max_dist > min_dist * 3.0f) && n_pairs >= 2;
  }
  accept[i] = ok ? 1u : 0u;
  if (!ok) return;
  uint32_t g0 = 0xffffffffu;
  for (uint32_t e = t0; e < t1; e++) {
    if (!in.cnt[e - sv_base]) continue;
    const uint32_t node = s.view_pl_off[sd.trk_view[e]] + in.pl[e - sv_base];
    if (g.first[node] > (unsigned long long)seed) atomicMin(g.first + node, (unsigned long long)seed);
    if (g0 == 0xffffffffu)
      g0 = node;
    else
      k9_unite(g.parent, g0, node);
  }
}

__global__ void __launch_bounds__(K9_BLOCK) k9_flatten(uint32_t n_pl, K9Graph g, uint32_t* n_nodes) {
  const uint32_t i = blockIdx.x * K9_BLOCK + threadIdx.x;
  const bool node = i < n_pl && g.first[i] != K9_NONE;
  if (node) {
    const uint32_t root = k9_find(g.parent, i);
    g.root_of[i] = root;
    atomicMin(g.ckey + root, (g.first[i] << 32) | (unsigned long long)i);
  }
  const uint32_t n = (uint32_t)__popcll(__ballot(node));
  if ((threadIdx.x & 63u) == 0 && n) atomicAdd(n_nodes, n);
}

__global__ void __launch_bounds__(K9_BLOCK) k9_rank(const unsigned long long* ckey_sorted, uint32_t n_pl, K9Graph g,
                                                    uint32_t* n_sets) {
  const uint32_t j = blockIdx.x * K9_BLOCK + threadIdx.x;
  const bool set = j < n_pl && ckey_sorted[j] != K9_NONE;
  if (set) g.rank_of[g.root_of[(uint32_t)ckey_sorted[j]]] = j;  // (the key's low word is a node of the component)
  const uint32_t n = (uint32_t)__popcll(__ballot(set));
  if ((threadIdx.x & 63u) == 0 && n) atomicAdd(n_sets, n);
}

__global__ void __launch_bounds__(K9_BLOCK) k9_node_keys(DevScene s, uint32_t n_pl, K9Graph g, unsigned long long* keys) {
  const uint32_t i = blockIdx.x * K9_BLOCK + threadIdx.x;
  if (i >= n_pl) return;
  unsigned long long key = K9_NONE;
  if (g.first[i] != K9_NONE) {
    uint32_t lo = 0, hi = (uint32_t)s.n_views;  // view of polyline i: last v with view_pl_off[v] <= i (as K0)
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s.view_pl_off[mid] <= i) lo = mid; else hi = mid;
    }
    const unsigned long long row = (unsigned long long)g.rank_of[g.root_of[i]] * (unsigned long long)s.n_views + lo;
    key = (row << EG3D_K0_PL_BITS_HOST) | (unsigned long long)(i - s.view_pl_off[lo]);
  }
  keys[i] = key;
}

__global__ void __launch_bounds__(K9_BLOCK) k9_compact(const uint32_t* accept, const uint32_t* off, uint32_t seed_begin,
                                                       uint32_t n_seeds, uint32_t* accepted) {
  const uint32_t i = blockIdx.x * K9_BLOCK + threadIdx.x;
  if (i < n_seeds && accept[i]) accepted[off[i]] = seed_begin + i;
}

// ------------------------------------------------------------ launch wrappers --
void launch_k9_prep(hipStream_t st, SeedsDev sd, int32_t n_views, uint32_t seed_begin, uint32_t n_seeds, uint32_t sv_base,
                    uint32_t* sv_seed, uint32_t* flags) {
  if (!n_seeds) return;
  hipLaunchKernelGGL(k9_prep, blocks_for(n_seeds, K9_BLOCK), dim3(K9_BLOCK), 0, st, sd, n_views, seed_begin, n_seeds, sv_base,
                     sv_seed, flags);
}
void launch_k9_close_polylines(hipStream_t st, DevScene s, K9Grid g10, SeedsDev sd, uint32_t sv_base, uint32_t n_sv,
                               const uint32_t* sv_seed, K9Entries out) {
  if (!n_sv) return;
  hipLaunchKernelGGL(k9_close_polylines, blocks_for((uint64_t)n_sv * 64, K9_BLOCK), dim3(K9_BLOCK), 0, st, s, g10, sd, sv_base,
                     n_sv, sv_seed, out);
}
void launch_k9_init(hipStream_t st, uint32_t n_pl, K9Graph g) {
  if (!n_pl) return;
  hipLaunchKernelGGL(k9_init, blocks_for(n_pl, K9_BLOCK), dim3(K9_BLOCK), 0, st, n_pl, g);
}
void launch_k9_refpoint_rule(hipStream_t st, DevScene s, SeedsDev sd, uint32_t seed_begin, uint32_t n_seeds, uint32_t sv_base,
                             K9Entries in, uint32_t* accept, K9Graph g) {
  hipLaunchKernelGGL(k9_refpoint_rule, blocks_for((uint64_t)n_seeds + 1, K9_BLOCK), dim3(K9_BLOCK), 0, st, s, sd, seed_begin,
                     n_seeds, sv_base, in, accept, g);
}
void launch_k9_flatten(hipStream_t st, uint32_t n_pl, K9Graph g, uint32_t* n_nodes) {
  if (!n_pl) return;
  hipLaunchKernelGGL(k9_flatten, blocks_for(n_pl, K9_BLOCK), dim3(K9_BLOCK), 0, st, n_pl, g, n_nodes);
}
void launch_k9_rank(hipStream_t st, const unsigned long long* ckey_sorted, uint32_t n_pl, K9Graph g, uint32_t* n_sets) {
  if (!n_pl) return;
  hipLaunchKernelGGL(k9_rank, blocks_for(n_pl, K9_BLOCK), dim3(K9_BLOCK), 0, st, ckey_sorted, n_pl, g, n_sets);
}
void launch_k9_node_keys(hipStream_t st, DevScene s, uint32_t n_pl, K9Graph g, unsigned long long* keys) {
  if (!n_pl) return;
  hipLaunchKernelGGL(k9_node_keys, blocks_for(n_pl, K9_BLOCK), dim3(K9_BLOCK), 0, st, s, n_pl, g, keys);
}
void launch_k9_compact(hipStream_t st, const uint32_t* accept, const uint32_t* off, uint32_t seed_begin, uint32_t n_seeds,
                       uint32_t* accepted) {
  if (!n_seeds) return;
  hipLaunchKernelGGL(k9_compact, blocks_for(n_seeds, K9_BLOCK), dim3(K9_BLOCK), 0, st, accept, off, seed_begin, n_seeds, accepted);
}

}  // namespace eg3d
