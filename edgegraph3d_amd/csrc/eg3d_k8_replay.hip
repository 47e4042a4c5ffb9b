// eg3d_k8_replay.hip — K8: the PLGMatchesManager replay on a device-resident cloud (eg3d_replay_device).
//
// host/replay.cpp is the sequential statement: every consecutive pair of chain points looks its two points up as nodes of
// the 3-D polyline graph (keyed by exact coordinates), connects them unless the connection exists in either orientation,
// and marks the 2-D interval between their observations on every view both see. Each of its order-dependent rules is a
// first-claim or a last-writer rule, so the passes below do not depend on the order in which lanes arrive:
//   * a pair is (i - 1, i) with equal key[0..2] and key[3] counting up by one; its two lookups have the orders 2 i and
//     2 i + 1. A point is looked up as the second of its own pair and as the first of the next, so the smallest (largest)
//     lookup order of a node belongs to the smallest (largest) POINT INDEX among the points with its coordinates;
//   * node id = rank of the node's first point among the first points; node_X = that point's X as stored (-0 stays -0);
//     node_point = the node's last point;
//   * polyline = distinct unordered pair {na, nb}; id = rank of its first pair; orientation of that pair;
//   * conn[node] = its polylines in ascending id (a polyline is linked to both ends when it is created: ascending id IS
//     insertion order);
//   * interval key = (scene polyline, start segment) = one entry of a map indexed by the scene's global segment index
//     pl_vtx_off[g] + seg; the first insertion in the order (pair, view ascending) wins = the minimum of
//     pair * n_views + view.
// What this does NOT restate is the reference's treatment of a NaN coordinate (never equal: a new node per lookup) and of
// x or y == -1 ("invalid" node: wiped when found again): k8_pairs detects both on the points that belong to pairs and the
// call is refused (EG3D_ERR_HOSTONLY) before any of the passes below runs.
//   k8_pairs         1 lane / point and / observation: every check (offsets, view, polyline, segment, NaN / -1), pair count
//   k8_node_claim    1 lane / point of a pair: open addressing, atomicCAS from empty, atomicMin on the slot (the slot's
//                    owner is replaced by a smaller index OF THE SAME coordinates, so probes that compare against the owner
//                    see the same key whoever owns it), atomicMax on the last-point word
//   k8_node_resolve  1 lane / point of a pair: first point of its node; flag at first points
//   k8_node_write    1 lane / point: node arrays, sort keys of the pairs          (rocPRIM: scan of the flags before it,
//   k8_pl_heads      1 lane / sorted pair: run heads create the polylines          stable 64-bit radix sort after it)
//   k8_pl_write      1 lane / point: polyline arrays and the (node, polyline) incidence keys  (sorted: conn)
//   k8_conn          1 lane / incidence: conn_pl, conn_off at the node boundaries
//   k8_iv<false>     8 lanes / pair: atomicMin of pair * n_views + view into the segment map (read first, as K7 does)
//   k8_iv<true>      the same walk: the winner writes its record at the scanned position of its segment
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "eg3d_k8_dev.h"
#include "eg3d_k8_replay.h"

namespace eg3d {

__global__ void __launch_bounds__(K8_BLOCK) k8_pairs(CloudView in, DevScene s, unsigned long long* n_pairs, uint32_t* flags) {
  const uint64_t t = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  uint32_t bad = 0;
  bool pair = false;
  if (t < in.n_points) {
    const uint64_t a = in.obs_off[t], b = t + 1 < in.n_points ? in.obs_off[t + 1] : in.n_obs;
    if (!(a <= b && b <= in.n_obs)) bad |= K8_FLAG_BAD_OFFSETS;
    pair = k8_is_pair(in, t);
    if (pair || k8_is_pair(in, t + 1)) {
      const float x = in.X[3 * t], y = in.X[3 * t + 1], z = in.X[3 * t + 2];
      if (x != x || y != y || z != z || x == -1.0f || y == -1.0f) bad |= K8_FLAG_HOSTONLY;
    }
  }
  if (t < in.n_obs) {
    const int32_t v = in.obs_view[t];
    if (v < 0 || v >= s.n_views)
      bad |= K8_FLAG_BAD_VIEW;
    else {
      const uint32_t g0 = s.view_pl_off[v], npl = s.view_pl_off[v + 1] - g0, pl = in.obs_pl[t];
      if (pl >= npl)
        bad |= K8_FLAG_BAD_PL;
      else {
        const uint32_t nv = s.pl_vtx_off[g0 + pl + 1] - s.pl_vtx_off[g0 + pl];
        if (nv < 2 || in.obs_seg[t] >= nv - 1) bad |= K8_FLAG_BAD_SEG;
      }
    }
  }
  if (bad) atomicOr(flags, bad);
  const uint32_t n = (uint32_t)__popcll(__ballot(pair));
  if ((threadIdx.x & 63u) == 0 && n) atomicAdd(n_pairs, (unsigned long long)n);
}

// ---- nodes ----
// The table has more slots than there are lookups, so a free slot always ends a probe sequence; the walks below are
// bounded by the table size all the same.
__global__ void __launch_bounds__(K8_BLOCK) k8_node_claim(CloudView in, K8Table t) {
  const uint64_t p = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (p >= in.n_points || !k8_in_pair(in, p)) return;
  const K8Key k = k8_key(in.X, p);
  uint64_t h = k8_hash(k) & t.mask;
  for (uint64_t step = 0; step <= t.mask; step++, h = (h + 1) & t.mask) {
    uint32_t cur = __hip_atomic_load(t.slot + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == K8_EMPTY) {
      cur = atomicCAS(t.slot + h, K8_EMPTY, (uint32_t)p);
      if (cur == K8_EMPTY) break;  // claimed
    }
    if (cur == (uint32_t)p || k8_same(k8_key(in.X, cur), k)) {
      if (cur > (uint32_t)p) atomicMin(t.slot + h, (uint32_t)p);  // (an owner only ever decreases: a smaller one cannot be lowered)
      break;
    }
  }
  if (__hip_atomic_load(t.last + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (uint32_t)p) atomicMax(t.last + h, (uint32_t)p);
}
__global__ void __launch_bounds__(K8_BLOCK) k8_node_resolve(CloudView in, K8Table t, uint32_t* first_of, uint32_t* is_first,
                                                           uint32_t* last_of) {
  const uint64_t p = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (p >= in.n_points || !k8_in_pair(in, p)) return;
  const K8Key k = k8_key(in.X, p);
  uint64_t h = k8_hash(k) & t.mask;
  uint32_t fp = (uint32_t)p;
  for (uint64_t step = 0; step <= t.mask; step++, h = (h + 1) & t.mask) {
    const uint32_t cur = t.slot[h];
    if (cur == K8_EMPTY) break;  // (unreachable: p claimed a slot of this sequence)
    if (cur == (uint32_t)p || k8_same(k8_key(in.X, cur), k)) {
      fp = cur;
      break;
    }
  }
  first_of[p] = fp;
  if (fp == (uint32_t)p) {
    is_first[p] = 1u;
    last_of[p] = t.last[h];
  }
}
__device__ __forceinline__ void k8_pair_nodes(const uint32_t* first_of, const uint32_t* rank, uint64_t i, uint32_t* na, uint32_t* nb) {
  *na = rank[first_of[i - 1]];
  *nb = rank[first_of[i]];
}
__global__ void __launch_bounds__(K8_BLOCK) k8_node_write(CloudView in, const uint32_t* first_of, const uint32_t* is_first,
                                                         const uint32_t* rank, const uint32_t* last_of, K8Graph g,
                                                         unsigned long long* pair_key, uint32_t* pair_val) {
  const uint64_t i = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (i >= in.n_points) return;
  if (is_first[i]) {
    const uint64_t id = rank[i];
    g.node_X[3 * id] = in.X[3 * i];
    g.node_X[3 * id + 1] = in.X[3 * i + 1];
    g.node_X[3 * id + 2] = in.X[3 * i + 2];
    g.node_point[id] = last_of[i];
  }
  unsigned long long key = ~0ull;
  if (k8_is_pair(in, i)) {
    uint32_t na, nb;
    k8_pair_nodes(first_of, rank, i, &na, &nb);
    key = ((unsigned long long)(na < nb ? na : nb) << 32) | (na < nb ? nb : na);
  }
  pair_key[i] = key;
  pair_val[i] = (uint32_t)i;
}

// ---- polylines and connections ----
__global__ void __launch_bounds__(K8_BLOCK) k8_pl_heads(const unsigned long long* key_sorted, const uint32_t* val_sorted,
                                                       uint64_t n_pairs, uint32_t* creates) {
  const uint64_t j = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (j >= n_pairs) return;
  if (j == 0 || key_sorted[j] != key_sorted[j - 1]) creates[val_sorted[j]] = 1u;
}
__global__ void __launch_bounds__(K8_BLOCK) k8_pl_write(CloudView in, const uint32_t* first_of, const uint32_t* rank,
                                                       const uint32_t* creates, const uint32_t* pl_id, K8Graph g,
                                                       unsigned long long* inc) {
  const uint64_t i = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (i >= in.n_points || !creates[i]) return;
  const uint64_t p = pl_id[i];
  uint32_t na, nb;
  k8_pair_nodes(first_of, rank, i, &na, &nb);
  g.pl_start[p] = na;
  g.pl_end[p] = nb;
  inc[2 * p] = ((unsigned long long)na << 32) | p;
  inc[2 * p + 1] = na != nb ? ((unsigned long long)nb << 32) | p : ~0ull;
}
__global__ void __launch_bounds__(K8_BLOCK) k8_conn(const unsigned long long* inc_sorted, uint64_t n_inc, uint64_t n_nodes,
                                                   K8Graph g) {
  const uint64_t j = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (j >= n_inc) return;
  const unsigned long long k = inc_sorted[j];
  if (k == ~0ull) return;
  g.conn_pl[j] = (uint32_t)k;
  const uint64_t node = k >> 32;
  if (node >= n_nodes) return;  // (unreachable)
  // the nodes from the previous entry's (exclusive) to this one's start here: every node has a connection, so normally one
  for (uint64_t n = j ? (inc_sorted[j - 1] >> 32) + 1 : 0; n <= node; n++) g.conn_off[n] = j;
  if (j + 1 == n_inc || inc_sorted[j + 1] == ~0ull)
    for (uint64_t n = node + 1; n <= n_nodes; n++) g.conn_off[n] = j + 1;
}

// ---- matched 2-D intervals ----
// 8 lanes per pair, 32 pairs per block (the shape of k7_dedup_keep: the lists of a matched cloud hold 3 to 9 observations).
// A lane takes the observations a1 + sub, a1 + sub + 8, ... of the first point; one counts when it is the LAST of its view
// in its list (slot[v] of the host pass), and meets the last observation of that view in the second point's list. The
// lists were validated by k8_pairs: every index below lies inside the scene.
template <bool WRITE>
__global__ void __launch_bounds__(K8_BLOCK) k8_iv(CloudView in, DevScene s, unsigned long long* map, const uint32_t* pos, K8Graph g) {
  const uint32_t t = threadIdx.x, sub = t & 7u;
  const uint64_t i = (uint64_t)blockIdx.x * (K8_BLOCK / 8) + (t >> 3);
  if (!k8_is_pair(in, i)) return;
  const uint64_t a1 = in.obs_off[i - 1], a2 = in.obs_off[i], b2 = i + 1 < in.n_points ? in.obs_off[i + 1] : in.n_obs;
  for (uint64_t o1 = a1 + sub; o1 < a2; o1 += 8) {
    const int32_t v = in.obs_view[o1];
    bool last = true;
    for (uint64_t o = o1 + 1; o < a2 && last; o++) last = in.obs_view[o] != v;
    if (!last) continue;
    uint64_t o2 = b2;
    while (o2 > a2 && in.obs_view[o2 - 1] != v) o2--;
    if (o2 == a2) continue;  // the second point does not see the view
    o2--;
    uint32_t gpl;
    K8Plp a, b;
    if (!k8_interval(in, s, v, o1, o2, &gpl, &a, &b)) continue;
    const uint64_t cell = (uint64_t)s.pl_vtx_off[gpl] + a.seg;
    const unsigned long long id = (unsigned long long)i * (unsigned long long)s.n_views + (unsigned long long)v;
    if constexpr (!WRITE) {
      // an entry only ever decreases: one that already reads <= id cannot be lowered by this lane
      if (map[cell] > id) atomicMin(map + cell, id);
    } else if (map[cell] == id) {
      const uint64_t k = pos[cell];
      g.iv_start_seg[k] = a.seg;
      g.iv_end_seg[k] = b.seg;
      g.iv_start_xy[2 * k] = a.x;
      g.iv_start_xy[2 * k + 1] = a.y;
      g.iv_end_xy[2 * k] = b.x;
      g.iv_end_xy[2 * k + 1] = b.y;
    }
  }
}
__global__ void __launch_bounds__(K8_BLOCK) k8_seg_flags(const unsigned long long* map, uint64_t n_vtx, uint32_t* flag) {
  const uint64_t j = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (j <= n_vtx) flag[j] = j < n_vtx && map[j] != K8_UNCLAIMED ? 1u : 0u;
}
__global__ void __launch_bounds__(K8_BLOCK) k8_iv_off(DevScene s, uint32_t n_pl, const uint32_t* pos, K8Graph g) {
  const uint64_t p = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (p <= n_pl) g.iv_off[p] = pos[s.pl_vtx_off[p]];
}

// ------------------------------------------------------------ launch wrappers --
void launch_k8_pairs(hipStream_t st, CloudView in, DevScene s, unsigned long long* n_pairs, uint32_t* flags) {
  const uint64_t n = in.n_points > in.n_obs ? in.n_points : in.n_obs;
  if (!n) return;
  hipLaunchKernelGGL(k8_pairs, blocks_for(n, K8_BLOCK), dim3(K8_BLOCK), 0, st, in, s, n_pairs, flags);
}
void launch_k8_node_claim(hipStream_t st, CloudView in, K8Table t) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k8_node_claim, blocks_for(in.n_points, K8_BLOCK), dim3(K8_BLOCK), 0, st, in, t);
}
void launch_k8_node_resolve(hipStream_t st, CloudView in, K8Table t, uint32_t* first_of, uint32_t* is_first, uint32_t* last_of) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k8_node_resolve, blocks_for(in.n_points, K8_BLOCK), dim3(K8_BLOCK), 0, st, in, t, first_of, is_first, last_of);
}
void launch_k8_node_write(hipStream_t st, CloudView in, const uint32_t* first_of, const uint32_t* is_first, const uint32_t* rank,
                          const uint32_t* last_of, K8Graph g, unsigned long long* pair_key, uint32_t* pair_val) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k8_node_write, blocks_for(in.n_points, K8_BLOCK), dim3(K8_BLOCK), 0, st, in, first_of, is_first, rank, last_of,
                     g, pair_key, pair_val);
}
void launch_k8_pl_heads(hipStream_t st, const unsigned long long* key_sorted, const uint32_t* val_sorted, uint64_t n_pairs,
                        uint32_t* creates) {
  if (!n_pairs) return;
  hipLaunchKernelGGL(k8_pl_heads, blocks_for(n_pairs, K8_BLOCK), dim3(K8_BLOCK), 0, st, key_sorted, val_sorted, n_pairs, creates);
}
void launch_k8_pl_write(hipStream_t st, CloudView in, const uint32_t* first_of, const uint32_t* rank, const uint32_t* creates,
                        const uint32_t* pl_id, K8Graph g, unsigned long long* inc) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k8_pl_write, blocks_for(in.n_points, K8_BLOCK), dim3(K8_BLOCK), 0, st, in, first_of, rank, creates, pl_id, g,
                     inc);
}
void launch_k8_conn(hipStream_t st, const unsigned long long* inc_sorted, uint64_t n_inc, uint64_t n_nodes, K8Graph g) {
  if (!n_inc) return;
  hipLaunchKernelGGL(k8_conn, blocks_for(n_inc, K8_BLOCK), dim3(K8_BLOCK), 0, st, inc_sorted, n_inc, n_nodes, g);
}
void launch_k8_iv(hipStream_t st, bool write, CloudView in, DevScene s, unsigned long long* map, const uint32_t* pos, K8Graph g) {
  if (!in.n_points) return;
  if (write)
    hipLaunchKernelGGL(k8_iv<true>, blocks_for(in.n_points, K8_BLOCK / 8), dim3(K8_BLOCK), 0, st, in, s, map, pos, g);
  else
    hipLaunchKernelGGL(k8_iv<false>, blocks_for(in.n_points, K8_BLOCK / 8), dim3(K8_BLOCK), 0, st, in, s, map, pos, g);
}
void launch_k8_seg_flags(hipStream_t st, const unsigned long long* map, uint64_t n_vtx, uint32_t* flag) {
  hipLaunchKernelGGL(k8_seg_flags, blocks_for(n_vtx + 1, K8_BLOCK), dim3(K8_BLOCK), 0, st, map, n_vtx, flag);
}
void launch_k8_iv_off(hipStream_t st, DevScene s, uint32_t n_pl, const uint32_t* pos, K8Graph g) {
  hipLaunchKernelGGL(k8_iv_off, blocks_for((uint64_t)n_pl + 1, K8_BLOCK), dim3(K8_BLOCK), 0, st, s, n_pl, pos, g);
}

hipError_t k8_scan_u32(hipStream_t st, void* tmp, size_t& tmp_bytes, const uint32_t* in, uint32_t* out, size_t n) {
  return rocprim::exclusive_scan(tmp, tmp_bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), st);
}
hipError_t k8_sort_pairs(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* key_in, unsigned long long* key_out,
                         const uint32_t* val_in, uint32_t* val_out, size_t n) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, key_in, key_out, val_in, val_out, n, 0, 64, st);
}
hipError_t k8_sort_keys(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* key_in, unsigned long long* key_out,
                        size_t n) {
  return rocprim::radix_sort_keys(tmp, tmp_bytes, key_in, key_out, n, 0, 64, st);
}

}  // namespace eg3d
