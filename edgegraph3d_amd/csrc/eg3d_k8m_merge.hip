// eg3d_k8m_merge.hip — K8m: the accumulator of the PLGMatchesManager replay (K8a, eg3d_k8a_accumulate.hip) takes the GRAPH of the
// run that follows in place of its cloud (eg3d_replay_merge_graph, include/eg3d_replay_merge.h). host/replay.cpp states the rule
// sequentially (eg3d_host_replay_state_merge_graph); here, with A the state of nA points and B the graph `later`:
//   * nodes: B's nodes have distinct canonical coordinates (checked), so each is its own "first point" of K8a's node pass:
//     k8a_node_lookup probes the state's table for every B node, a miss is new with id = A's nodes + rank among the misses in B's
//     id order, and k8a_node_write appends node_X as B stores it and sets node_point = nA + B.node_point for settled and new
//     nodes alike (B's points all come after A's). node_id[b] is then the map from B's ids to the merged ids, and it is injective;
//   * polylines: the keys min << 32 | max of B's polylines with their endpoints mapped are sorted stably and go through
//     k8a_pl_heads against the persistent keys; B's polylines are distinct (checked), so every key heads its own run and
//     creates exactly when A does not hold it. New ids = A's polylines + scan in B's id order, in B's orientation;
//   * intervals: a cell of the claim map that nobody holds takes B's record. The claim id is nA * n_views: not K8_UNCLAIMED
//     and below every id a later cloud can produce ((nA + nB + i) * n_views + view with i >= 1), and K8a's claim pass never
//     lowers a claimed cell to a later id. B's rows name a cell at most once (checked), so one lane per interval needs no atomic
//     on the map.
// Nothing of B is used as an index before the checks have passed, in two steps because the second indexes with the first's
// results: k8m_check (node_point, endpoints, NaN / -1, the interval offsets against the scene's segment counts), then
// k8m_iv_check (the segments of every interval), k8m_node_group (duplicates among B's nodes, on K8's scratch table) and
// k8m_pl_keys + sort + k8m_pl_dups (duplicates among B's polylines).
//   k8m_check       1 lane / node, / polyline and / scene polyline
//   k8m_iv_check    1 lane / interval
//   k8m_node_group  1 lane / node: atomicCAS from empty along the probe sequence, compare where it is taken
//   k8m_pl_keys     1 lane / polyline
//   k8m_pl_dups     1 lane / sorted key
//   k8m_pl_write    1 lane / polyline
//   k8m_iv          1 lane / interval
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "eg3d_k8_dev.h"
#include "eg3d_k8m_merge.h"

namespace eg3d {

// segments of scene polyline g (one with fewer than two vertices has none)
__device__ __forceinline__ uint32_t k8m_segments(const DevScene& s, uint32_t g) {
  const uint32_t nv = s.pl_vtx_off[g + 1] - s.pl_vtx_off[g];
  return nv < 2 ? 0u : nv - 1;
}
// the scene polyline whose row holds interval k: the last g < n with iv_off[g] <= k (iv_off ascends from 0 and k < iv_off[n])
__device__ __forceinline__ uint32_t k8m_row_of(const unsigned long long* iv_off, uint32_t n, uint64_t k) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (iv_off[mid] <= k)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(K8_BLOCK) k8m_check(K8mGraph b, DevScene s, uint32_t n_scene_pl, uint64_t later_points,
                                                     uint32_t* flags) {
  const uint64_t t = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  uint32_t bad = 0;
  if (t < b.n_nodes) {
    if (b.node_point[t] >= later_points) bad |= K8M_FLAG_BAD_POINT;
    const float x = b.node_X[3 * t], y = b.node_X[3 * t + 1], z = b.node_X[3 * t + 2];
    if (x != x || y != y || z != z || x == -1.0f || y == -1.0f) bad |= K8M_FLAG_HOSTONLY;
  }
  if (t < b.n_pl && (b.pl_start[t] >= b.n_nodes || b.pl_end[t] >= b.n_nodes)) bad |= K8M_FLAG_BAD_ENDPOINT;
  if (t < n_scene_pl) {
    const unsigned long long a = b.iv_off[t], e = b.iv_off[t + 1];
    if ((t == 0 && a != 0) || a > e || e - a > k8m_segments(s, (uint32_t)t)) bad |= K8M_FLAG_BAD_OFFSETS;
  }
  if (bad) atomicOr(flags, bad);
}
__global__ void __launch_bounds__(K8_BLOCK) k8m_iv_check(K8mGraph b, DevScene s, uint32_t n_scene_pl, uint64_t n_iv, uint32_t* flags) {
  const uint64_t k = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (k >= n_iv) return;
  const uint32_t g = k8m_row_of(b.iv_off, n_scene_pl, k), segs = k8m_segments(s, g);
  const uint32_t ss = b.iv_start_seg[k];
  uint32_t bad = 0;
  if (ss >= segs || b.iv_end_seg[k] >= segs) bad |= K8M_FLAG_BAD_SEG;
  if (k > b.iv_off[g] && b.iv_start_seg[k - 1] >= ss) bad |= K8M_FLAG_SEG_ORDER;
  if (bad) atomicOr(flags, bad);
}

// ---- nodes ----
// The table has more slots than B has nodes, so a free slot always ends a probe sequence; the walk is bounded by the table
// size all the same. Of two nodes with one key, the one that arrives second at the slot the first took sees it there.
__global__ void __launch_bounds__(K8_BLOCK) k8m_node_group(K8mGraph b, K8aTable t, uint32_t* every, uint32_t* last_of, uint32_t* flags) {
  const uint64_t n = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (n >= b.n_nodes) return;
  every[n] = 1u;
  last_of[n] = (uint32_t)b.node_point[n];
  const K8Key k = k8_key(b.node_X, n);
  uint64_t h = k8_hash(k) & t.mask;
  for (uint64_t step = 0; step <= t.mask; step++, h = (h + 1) & t.mask) {
    const uint32_t cur = atomicCAS(t.slot + h, K8_EMPTY, (uint32_t)n);
    if (cur == K8_EMPTY) break;
    if (cur < b.n_nodes && k8_same(k8_key(b.node_X, cur), k)) {
      atomicOr(flags, K8M_FLAG_DUP_NODE);
      break;
    }
  }
}

// ---- polylines ----
__global__ void __launch_bounds__(K8_BLOCK) k8m_pl_keys(K8mGraph b, const uint32_t* node_id, unsigned long long* key, uint32_t* val) {
  const uint64_t j = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (j >= b.n_pl) return;
  uint32_t na = b.pl_start[j], nb = b.pl_end[j];
  if (node_id) {
    na = node_id[na];
    nb = node_id[nb];
  }
  key[j] = ((unsigned long long)(na < nb ? na : nb) << 32) | (na < nb ? nb : na);
  val[j] = (uint32_t)j;
}
__global__ void __launch_bounds__(K8_BLOCK) k8m_pl_dups(const unsigned long long* key_sorted, uint64_t n, uint32_t* flags) {
  const uint64_t j = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (j == 0 || j >= n) return;
  if (key_sorted[j] == key_sorted[j - 1]) atomicOr(flags, K8M_FLAG_DUP_PL);
}
__global__ void __launch_bounds__(K8_BLOCK) k8m_pl_write(K8mGraph b, const uint32_t* node_id, const uint32_t* creates,
                                                        const uint32_t* pl_id, uint64_t n_pl, uint32_t* pl_start, uint32_t* pl_end,
                                                        unsigned long long* pl_key) {
  const uint64_t j = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (j >= b.n_pl || !creates[j]) return;
  const uint64_t p = n_pl + pl_id[j];
  const uint32_t na = node_id[b.pl_start[j]], nb = node_id[b.pl_end[j]];
  pl_start[p] = na;
  pl_end[p] = nb;
  pl_key[p] = ((unsigned long long)(na < nb ? na : nb) << 32) | (na < nb ? nb : na);
}

// ---- matched 2-D intervals ----
__global__ void __launch_bounds__(K8_BLOCK) k8m_iv(K8mGraph b, DevScene s, uint32_t n_scene_pl, uint64_t n_iv, unsigned long long id,
                                                  unsigned long long* map, K8aRecords r, unsigned long long* n_iv_state) {
  const uint64_t k = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (k >= n_iv) return;
  const uint32_t g = k8m_row_of(b.iv_off, n_scene_pl, k), ss = b.iv_start_seg[k];
  const uint64_t cell = (uint64_t)s.pl_vtx_off[g] + ss;
  if (map[cell] != K8_UNCLAIMED) return;  // A's record stands
  map[cell] = id;
  r.start_seg[cell] = ss;
  r.end_seg[cell] = b.iv_end_seg[k];
  r.start_xy[2 * cell] = b.iv_start_xy[2 * k];
  r.start_xy[2 * cell + 1] = b.iv_start_xy[2 * k + 1];
  r.end_xy[2 * cell] = b.iv_end_xy[2 * k];
  r.end_xy[2 * cell + 1] = b.iv_end_xy[2 * k + 1];
  atomicAdd(n_iv_state, 1ull);
}

// ------------------------------------------------------------ launch wrappers --
void launch_k8m_check(hipStream_t st, K8mGraph b, DevScene s, uint32_t n_scene_pl, uint64_t later_points, uint32_t* flags) {
  const uint64_t n = std::max<uint64_t>(std::max<uint64_t>(b.n_nodes, b.n_pl), n_scene_pl);
  if (!n) return;
  hipLaunchKernelGGL(k8m_check, blocks_for(n, K8_BLOCK), dim3(K8_BLOCK), 0, st, b, s, n_scene_pl, later_points, flags);
}
void launch_k8m_iv_check(hipStream_t st, K8mGraph b, DevScene s, uint32_t n_scene_pl, uint64_t n_iv, uint32_t* flags) {
  if (!n_iv) return;
  hipLaunchKernelGGL(k8m_iv_check, blocks_for(n_iv, K8_BLOCK), dim3(K8_BLOCK), 0, st, b, s, n_scene_pl, n_iv, flags);
}
void launch_k8m_node_group(hipStream_t st, K8mGraph b, K8aTable t, uint32_t* every, uint32_t* last_of, uint32_t* flags) {
  if (!b.n_nodes) return;
  hipLaunchKernelGGL(k8m_node_group, blocks_for(b.n_nodes, K8_BLOCK), dim3(K8_BLOCK), 0, st, b, t, every, last_of, flags);
}
void launch_k8m_pl_keys(hipStream_t st, K8mGraph b, const uint32_t* node_id, unsigned long long* key, uint32_t* val) {
  if (!b.n_pl) return;
  hipLaunchKernelGGL(k8m_pl_keys, blocks_for(b.n_pl, K8_BLOCK), dim3(K8_BLOCK), 0, st, b, node_id, key, val);
}
void launch_k8m_pl_dups(hipStream_t st, const unsigned long long* key_sorted, uint64_t n, uint32_t* flags) {
  if (n < 2) return;
  hipLaunchKernelGGL(k8m_pl_dups, blocks_for(n, K8_BLOCK), dim3(K8_BLOCK), 0, st, key_sorted, n, flags);
}
void launch_k8m_pl_write(hipStream_t st, K8mGraph b, const uint32_t* node_id, const uint32_t* creates, const uint32_t* pl_id,
                         uint64_t n_pl, uint32_t* pl_start, uint32_t* pl_end, unsigned long long* pl_key) {
  if (!b.n_pl) return;
  hipLaunchKernelGGL(k8m_pl_write, blocks_for(b.n_pl, K8_BLOCK), dim3(K8_BLOCK), 0, st, b, node_id, creates, pl_id, n_pl, pl_start,
                     pl_end, pl_key);
}
void launch_k8m_iv(hipStream_t st, K8mGraph b, DevScene s, uint32_t n_scene_pl, uint64_t n_iv, unsigned long long id,
                   unsigned long long* map, K8aRecords r, unsigned long long* n_iv_state) {
  if (!n_iv) return;
  hipLaunchKernelGGL(k8m_iv, blocks_for(n_iv, K8_BLOCK), dim3(K8_BLOCK), 0, st, b, s, n_scene_pl, n_iv, id, map, r, n_iv_state);
}

}  // namespace eg3d
