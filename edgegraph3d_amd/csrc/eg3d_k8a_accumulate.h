// Host-visible declarations of K8a (eg3d_k8a_accumulate.hip): the PLGMatchesManager replay that accumulates over the clouds of
// a run (eg3d_replay_accumulate). The checks, the grouping of a cloud's own points, the connections and the interval offsets
// are K8's kernels (eg3d_k8_replay.h), launched unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_k8_replay.h"

namespace eg3d {

// The state's node table: open addressing over `mask + 1` slots (a power of two); slot = a settled node id, compared through
// the state's node_X (K8_EMPTY: free).
struct K8aTable {
  uint32_t* slot;
  uint64_t mask;
};
// The interval records of the state, dense over the scene's global segment index (valid where the claim map is claimed).
struct K8aRecords {
  uint32_t* start_seg;
  uint32_t* end_seg;
  float* start_xy;
  float* end_xy;
};

// the node ids [id0, id1) into the table (all of them after a rehash; the table was filled with K8_EMPTY before)
void launch_k8a_table_insert(hipStream_t st, K8aTable t, const float* node_X, uint64_t id0, uint64_t id1);
// every first point of the cloud (is_first of launch_k8_node_resolve): node_id[p] = the settled node of its coordinates, or
// K8_EMPTY and is_new[p] = 1 (zeroed before)
void launch_k8a_node_lookup(hipStream_t st, CloudView in, K8aTable t, const float* node_X, const uint32_t* is_first, uint32_t* node_id,
                            uint32_t* is_new);
// rank = exclusive scan of is_new. New nodes: id = n_nodes + rank, node_X appended, id inserted into the table, node_id[p]
// set; every first point: node_point[its node] = base + last_of[p]. node_X / node_point hold n_nodes + (number of new) entries.
void launch_k8a_node_write(hipStream_t st, CloudView in, const uint32_t* is_first, const uint32_t* is_new, const uint32_t* rank,
                           const uint32_t* last_of, uint64_t base, uint64_t n_nodes, uint32_t* node_id, float* node_X,
                           unsigned long long* node_point, K8aTable t);
// per point i the sort key of its pair (min(na, nb) << 32 | max(na, nb); ~0 where i closes no pair) with the value i
void launch_k8a_pair_keys(hipStream_t st, CloudView in, const uint32_t* first_of, const uint32_t* node_id, unsigned long long* pair_key,
                          uint32_t* pair_val);
// over the sorted keys: the first pair of a run whose key is not among the n_pl sorted keys pl_key -> creates[pair] = 1
void launch_k8a_pl_heads(hipStream_t st, const unsigned long long* key_sorted, const uint32_t* val_sorted, uint64_t n_pairs,
                         const unsigned long long* pl_key, uint64_t n_pl, uint32_t* creates);
// pl_id = exclusive scan of creates: polyline n_pl + pl_id[i] gets pl_start / pl_end / pl_key of the creating pair i
void launch_k8a_pl_write(hipStream_t st, CloudView in, const uint32_t* first_of, const uint32_t* node_id, const uint32_t* creates,
                         const uint32_t* pl_id, uint64_t n_pl, uint32_t* pl_start, uint32_t* pl_end, unsigned long long* pl_key);
// inc[2 p] = pl_start[p] << 32 | p, inc[2 p + 1] = pl_end[p] << 32 | p (~0 for a loop): sorted, the input of launch_k8_conn
void launch_k8a_inc(hipStream_t st, const uint32_t* pl_start, const uint32_t* pl_end, uint64_t n_pl, unsigned long long* inc);
// write = false: the 64-bit minimum of (base + pair) * n_views + view into map[global start segment]; write = true: the ids
// of this cloud that stand write their records at the cell and add one to *n_iv
void launch_k8a_iv(hipStream_t st, bool write, CloudView in, DevScene s, uint64_t base, unsigned long long* map, K8aRecords r,
                   unsigned long long* n_iv);
// the record of every claimed cell to pos[cell] of the graph's interval arrays
void launch_k8a_iv_gather(hipStream_t st, const unsigned long long* map, uint64_t n_vtx, const uint32_t* pos, K8aRecords r, K8Graph g);

}  // namespace eg3d
