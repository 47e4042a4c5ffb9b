// eg3d_k8a_accumulate.hip — K8a: the PLGMatchesManager replay as a state that takes the clouds of a run one after the other
// (eg3d_replay_accumulate, include/eg3d_accumulate.h). K8 (eg3d_k8_replay.hip) needs the whole matched cloud; here the
// points of a cloud count from the number of points added before it, and what an earlier cloud decided is never revised —
// every order-dependent rule is a first-claim or a last-writer rule over those numbers:
//   * nodes: the node table of the STATE maps canonical (x, y, z) to a settled node id and compares through the persistent,
//     append-only node_X. A cloud first groups its own points with K8's kernels (k8_node_claim / k8_node_resolve, on K8's
//     scratch table: first point, last point of every key within the cloud); only the first points then look the state's
//     table up. A hit is a settled node: its node_point becomes the cloud's last point of that key (a later cloud's points
//     are all larger, and one lane per key writes). A miss is a new node: id = nodes so far + rank among the cloud's misses
//     (= order of first points, as the one-shot replay numbers them), node_X = that point's X as stored, and the id goes
//     into the table (insertions only in that pass: keys are distinct, so an insertion never compares);
//   * polylines: the sorted (min << 32 | max) keys of the polylines so far persist. The cloud's pairs are sorted stably as
//     in K8; a run head creates a polyline only if a binary search of the persistent keys misses. New ids = polylines so far
//     + scan; pl_start / pl_end in the creating pair's orientation are appended, the new keys are appended and the keys
//     sorted again;
//   * intervals: the claim map over the scene's vertices persists and holds the 64-bit minimum of
//     (points before + i) * n_views + view. An id of this cloud that stands after the claim pass took a cell that no earlier
//     cloud had claimed (theirs are all smaller): it writes its record into dense per-cell arrays and counts one interval.
// Asking for the graph (eg3d_api_accumulate.hip) derives the connections from pl_start / pl_end (k8a_inc, sort, K8's
// k8_conn) and gathers the claimed cells' records into the CSR (K8's k8_seg_flags, scan, k8a_iv_gather, K8's k8_iv_off);
// nothing of the state is written by it.
//   k8a_table_insert  1 lane / node id: atomicCAS from empty along the probe sequence
//   k8a_node_lookup   1 lane / first point of the cloud: probe the state's table, compare through node_X
//   k8a_node_write    1 lane / first point: new nodes appended and inserted, node_point of new and settled nodes
//   k8a_pair_keys     1 lane / point: the sort keys of the pairs
//   k8a_pl_heads      1 lane / sorted pair: run heads that the persistent keys do not hold create
//   k8a_pl_write      1 lane / point: the created polylines and their keys, appended
//   k8a_inc           1 lane / polyline: the (node, polyline) incidence keys
//   k8a_iv<false>     8 lanes / pair: atomicMin of the global id into the claim map (read first, as K7 and K8 do)
//   k8a_iv<true>      the same walk: this cloud's winners write their records and are counted
//   k8a_iv_gather     1 lane / scene vertex: the record of a claimed cell to its scanned position
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_k8_dev.h"
#include "eg3d_k8a_accumulate.h"

namespace eg3d {

// ---- nodes ----
// The table has more slots than the state has nodes, so a free slot always ends a probe sequence; the walks are bounded by
// the table size all the same.
__global__ void __launch_bounds__(K8_BLOCK) k8a_table_insert(K8aTable t, const float* node_X, uint64_t id0, uint64_t id1) {
  const uint64_t id = id0 + (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (id >= id1) return;
  uint64_t h = k8_hash(k8_key(node_X, id)) & t.mask;
  for (uint64_t step = 0; step <= t.mask; step++, h = (h + 1) & t.mask)
    if (atomicCAS(t.slot + h, K8_EMPTY, (uint32_t)id) == K8_EMPTY) break;
}
__global__ void __launch_bounds__(K8_BLOCK) k8a_node_lookup(CloudView in, K8aTable t, const float* node_X, const uint32_t* is_first,
                                                           uint32_t* node_id, uint32_t* is_new) {
  const uint64_t p = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (p >= in.n_points || !is_first[p]) return;
  const K8Key k = k8_key(in.X, p);
  uint64_t h = k8_hash(k) & t.mask;
  uint32_t id = K8_EMPTY;
  for (uint64_t step = 0; step <= t.mask; step++, h = (h + 1) & t.mask) {
    const uint32_t cur = t.slot[h];
    if (cur == K8_EMPTY) break;
    if (k8_same(k8_key(node_X, cur), k)) {
      id = cur;
      break;
    }
  }
  node_id[p] = id;
  if (id == K8_EMPTY) is_new[p] = 1u;
}
__global__ void __launch_bounds__(K8_BLOCK) k8a_node_write(CloudView in, const uint32_t* is_first, const uint32_t* is_new,
                                                          const uint32_t* rank, const uint32_t* last_of, uint64_t base,
                                                          uint64_t n_nodes, uint32_t* node_id, float* node_X,
                                                          unsigned long long* node_point, K8aTable t) {
  const uint64_t p = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (p >= in.n_points || !is_first[p]) return;
  uint64_t id = node_id[p];
  if (is_new[p]) {
    id = n_nodes + rank[p];
    node_id[p] = (uint32_t)id;
    node_X[3 * id] = in.X[3 * p];
    node_X[3 * id + 1] = in.X[3 * p + 1];
    node_X[3 * id + 2] = in.X[3 * p + 2];
    uint64_t h = k8_hash(k8_key(in.X, p)) & t.mask;
    for (uint64_t step = 0; step <= t.mask; step++, h = (h + 1) & t.mask)
      if (atomicCAS(t.slot + h, K8_EMPTY, (uint32_t)id) == K8_EMPTY) break;
  }
  node_point[id] = base + last_of[p];  // the last point of the node so far: every point of this cloud is later than the earlier clouds'
}
__global__ void __launch_bounds__(K8_BLOCK) k8a_pair_keys(CloudView in, const uint32_t* first_of, const uint32_t* node_id,
                                                         unsigned long long* pair_key, uint32_t* pair_val) {
  const uint64_t i = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (i >= in.n_points) return;
  unsigned long long key = ~0ull;
  if (k8_is_pair(in, i)) {
    const uint32_t na = node_id[first_of[i - 1]], nb = node_id[first_of[i]];
    key = ((unsigned long long)(na < nb ? na : nb) << 32) | (na < nb ? nb : na);
  }
  pair_key[i] = key;
  pair_val[i] = (uint32_t)i;
}

// ---- polylines and connections ----
__global__ void __launch_bounds__(K8_BLOCK) k8a_pl_heads(const unsigned long long* key_sorted, const uint32_t* val_sorted,
                                                        uint64_t n_pairs, const unsigned long long* pl_key, uint64_t n_pl,
                                                        uint32_t* creates) {
  const uint64_t j = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (j >= n_pairs) return;
  const unsigned long long k = key_sorted[j];
  if (j && k == key_sorted[j - 1]) return;
  uint64_t lo = 0, hi = n_pl;  // the first persistent key >= k
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (pl_key[mid] < k)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo < n_pl && pl_key[lo] == k) return;  // a polyline of an earlier cloud
  creates[val_sorted[j]] = 1u;
}
__global__ void __launch_bounds__(K8_BLOCK) k8a_pl_write(CloudView in, const uint32_t* first_of, const uint32_t* node_id,
                                                        const uint32_t* creates, const uint32_t* pl_id, uint64_t n_pl,
                                                        uint32_t* pl_start, uint32_t* pl_end, unsigned long long* pl_key) {
  const uint64_t i = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (i >= in.n_points || !creates[i]) return;
  const uint64_t p = n_pl + pl_id[i];
  const uint32_t na = node_id[first_of[i - 1]], nb = node_id[first_of[i]];  // (creates[i] is set at pairs only: i >= 1)
  pl_start[p] = na;
  pl_end[p] = nb;
  pl_key[p] = ((unsigned long long)(na < nb ? na : nb) << 32) | (na < nb ? nb : na);
}
__global__ void __launch_bounds__(K8_BLOCK) k8a_inc(const uint32_t* pl_start, const uint32_t* pl_end, uint64_t n_pl,
                                                   unsigned long long* inc) {
  const uint64_t p = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (p >= n_pl) return;
  const uint32_t na = pl_start[p], nb = pl_end[p];
  inc[2 * p] = ((unsigned long long)na << 32) | p;
  inc[2 * p + 1] = na != nb ? ((unsigned long long)nb << 32) | p : ~0ull;
}

// ---- matched 2-D intervals ----
// The walk of k8_iv (8 lanes per pair; the lists were validated by k8_pairs before anything of the state was touched).
template <bool WRITE>
__global__ void __launch_bounds__(K8_BLOCK) k8a_iv(CloudView in, DevScene s, uint64_t base, unsigned long long* map, K8aRecords r,
                                                  unsigned long long* n_iv) {
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
    const unsigned long long id = (unsigned long long)(base + i) * (unsigned long long)s.n_views + (unsigned long long)v;
    if constexpr (!WRITE) {
      // an entry only ever decreases: one that already reads <= id (an earlier cloud's always does) cannot be lowered
      if (map[cell] > id) atomicMin(map + cell, id);
    } else if (map[cell] == id) {
      r.start_seg[cell] = a.seg;
      r.end_seg[cell] = b.seg;
      r.start_xy[2 * cell] = a.x;
      r.start_xy[2 * cell + 1] = a.y;
      r.end_xy[2 * cell] = b.x;
      r.end_xy[2 * cell + 1] = b.y;
      atomicAdd(n_iv, 1ull);
    }
  }
}
__global__ void __launch_bounds__(K8_BLOCK) k8a_iv_gather(const unsigned long long* map, uint64_t n_vtx, const uint32_t* pos,
                                                         K8aRecords r, K8Graph g) {
  const uint64_t cell = (uint64_t)blockIdx.x * K8_BLOCK + threadIdx.x;
  if (cell >= n_vtx || map[cell] == K8_UNCLAIMED) return;
  const uint64_t k = pos[cell];
  g.iv_start_seg[k] = r.start_seg[cell];
  g.iv_end_seg[k] = r.end_seg[cell];
  g.iv_start_xy[2 * k] = r.start_xy[2 * cell];
  g.iv_start_xy[2 * k + 1] = r.start_xy[2 * cell + 1];
  g.iv_end_xy[2 * k] = r.end_xy[2 * cell];
  g.iv_end_xy[2 * k + 1] = r.end_xy[2 * cell + 1];
}

// ------------------------------------------------------------ launch wrappers --
void launch_k8a_table_insert(hipStream_t st, K8aTable t, const float* node_X, uint64_t id0, uint64_t id1) {
  if (id1 <= id0) return;
  hipLaunchKernelGGL(k8a_table_insert, blocks_for(id1 - id0, K8_BLOCK), dim3(K8_BLOCK), 0, st, t, node_X, id0, id1);
}
void launch_k8a_node_lookup(hipStream_t st, CloudView in, K8aTable t, const float* node_X, const uint32_t* is_first, uint32_t* node_id,
                            uint32_t* is_new) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k8a_node_lookup, blocks_for(in.n_points, K8_BLOCK), dim3(K8_BLOCK), 0, st, in, t, node_X, is_first, node_id, is_new);
}
void launch_k8a_node_write(hipStream_t st, CloudView in, const uint32_t* is_first, const uint32_t* is_new, const uint32_t* rank,
                           const uint32_t* last_of, uint64_t base, uint64_t n_nodes, uint32_t* node_id, float* node_X,
                           unsigned long long* node_point, K8aTable t) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k8a_node_write, blocks_for(in.n_points, K8_BLOCK), dim3(K8_BLOCK), 0, st, in, is_first, is_new, rank, last_of,
                     base, n_nodes, node_id, node_X, node_point, t);
}
void launch_k8a_pair_keys(hipStream_t st, CloudView in, const uint32_t* first_of, const uint32_t* node_id, unsigned long long* pair_key,
                          uint32_t* pair_val) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k8a_pair_keys, blocks_for(in.n_points, K8_BLOCK), dim3(K8_BLOCK), 0, st, in, first_of, node_id, pair_key, pair_val);
}
void launch_k8a_pl_heads(hipStream_t st, const unsigned long long* key_sorted, const uint32_t* val_sorted, uint64_t n_pairs,
                         const unsigned long long* pl_key, uint64_t n_pl, uint32_t* creates) {
  if (!n_pairs) return;
  hipLaunchKernelGGL(k8a_pl_heads, blocks_for(n_pairs, K8_BLOCK), dim3(K8_BLOCK), 0, st, key_sorted, val_sorted, n_pairs, pl_key, n_pl,
                     creates);
}
void launch_k8a_pl_write(hipStream_t st, CloudView in, const uint32_t* first_of, const uint32_t* node_id, const uint32_t* creates,
                         const uint32_t* pl_id, uint64_t n_pl, uint32_t* pl_start, uint32_t* pl_end, unsigned long long* pl_key) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k8a_pl_write, blocks_for(in.n_points, K8_BLOCK), dim3(K8_BLOCK), 0, st, in, first_of, node_id, creates, pl_id,
                     n_pl, pl_start, pl_end, pl_key);
}
void launch_k8a_inc(hipStream_t st, const uint32_t* pl_start, const uint32_t* pl_end, uint64_t n_pl, unsigned long long* inc) {
  if (!n_pl) return;
  hipLaunchKernelGGL(k8a_inc, blocks_for(n_pl, K8_BLOCK), dim3(K8_BLOCK), 0, st, pl_start, pl_end, n_pl, inc);
}
void launch_k8a_iv(hipStream_t st, bool write, CloudView in, DevScene s, uint64_t base, unsigned long long* map, K8aRecords r,
                   unsigned long long* n_iv) {
  if (!in.n_points) return;
  if (write)
    hipLaunchKernelGGL(k8a_iv<true>, blocks_for(in.n_points, K8_BLOCK / 8), dim3(K8_BLOCK), 0, st, in, s, base, map, r, n_iv);
  else
    hipLaunchKernelGGL(k8a_iv<false>, blocks_for(in.n_points, K8_BLOCK / 8), dim3(K8_BLOCK), 0, st, in, s, base, map, r, n_iv);
}
void launch_k8a_iv_gather(hipStream_t st, const unsigned long long* map, uint64_t n_vtx, const uint32_t* pos, K8aRecords r, K8Graph g) {
  if (!n_vtx) return;
  hipLaunchKernelGGL(k8a_iv_gather, blocks_for(n_vtx, K8_BLOCK), dim3(K8_BLOCK), 0, st, map, n_vtx, pos, r, g);
}

}  // namespace eg3d
