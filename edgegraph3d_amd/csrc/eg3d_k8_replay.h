// Host-visible declarations of K8 (eg3d_k8_replay.hip): the PLGMatchesManager replay (row a17) on a device-resident cloud.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_kernels.h"

namespace eg3d {

// what k8_pairs ORs into its flag word: the first two are the filter stage's (K5_FLAG_BAD_VIEW, K5_FLAG_BAD_OFFSETS)
enum : uint32_t { K8_FLAG_BAD_VIEW = 1u, K8_FLAG_BAD_OFFSETS = 2u, K8_FLAG_BAD_PL = 4u /* a polyline id outside its view */,
                  K8_FLAG_BAD_SEG = 8u /* a segment index outside its polyline, or a polyline without segments */,
                  K8_FLAG_HOSTONLY = 16u /* a NaN coordinate, or x or y == -1, in the X of a point that belongs to a pair */ };
#define K8_BLOCK 256
#define K8_EMPTY 0xFFFFFFFFu      /* node table: a free slot (point indices stay below 0xfffffff0) */
#define K8_UNCLAIMED (~0ull)      /* interval map: a segment no interval starts on */

// The node table: open addressing over `mask + 1` slots (a power of two). slot = the SMALLEST index of the points whose
// canonical (x, y, z) the slot holds (K8_EMPTY: free), last = the largest (zero-filled before the claims).
struct K8Table {
  uint32_t* slot;
  uint32_t* last;
  uint64_t mask;
};
// The result on the device: the members of eg3d_graph3d (include/eg3d_host.h) that are arrays.
struct K8Graph {
  float* node_X;
  unsigned long long* node_point;
  uint32_t* pl_start;
  uint32_t* pl_end;
  unsigned long long* conn_off;
  uint32_t* conn_pl;
  unsigned long long* iv_off;
  uint32_t* iv_start_seg;
  float* iv_start_xy;
  uint32_t* iv_end_seg;
  float* iv_end_xy;
};

// (1) the checks and the number of chain pairs: one lane per point AND per observation. *n_pairs and *flags zeroed before.
void launch_k8_pairs(hipStream_t st, CloudView in, DevScene s, unsigned long long* n_pairs, uint32_t* flags);
// (2) every point of a pair claims the slot of its coordinates; (3) reads it back: first_of[p] = the first point of p's
//     node, and for that first point is_first[p] = 1 (zeroed before) and last_of[p] = the node's last point
void launch_k8_node_claim(hipStream_t st, CloudView in, K8Table t);
void launch_k8_node_resolve(hipStream_t st, CloudView in, K8Table t, uint32_t* first_of, uint32_t* is_first, uint32_t* last_of);
// (4) rank = exclusive scan of is_first: the node ids. node_X / node_point of every node, and per point i the sort key of
//     its pair (min(na, nb) << 32 | max(na, nb); ~0 where i closes no pair) with the value i
void launch_k8_node_write(hipStream_t st, CloudView in, const uint32_t* first_of, const uint32_t* is_first, const uint32_t* rank,
                          const uint32_t* last_of, K8Graph g, unsigned long long* pair_key, uint32_t* pair_val);
// (5) over the sorted keys: the first pair of every run creates the polyline -> creates[pair] = 1 (zeroed before)
void launch_k8_pl_heads(hipStream_t st, const unsigned long long* key_sorted, const uint32_t* val_sorted, uint64_t n_pairs,
                        uint32_t* creates);
// (6) pl_id = exclusive scan of creates: pl_start / pl_end in the orientation of the creating pair, and the incidence keys
//     inc[2 p] = na << 32 | p, inc[2 p + 1] = nb << 32 | p (~0 for a loop, which is linked once)
void launch_k8_pl_write(hipStream_t st, CloudView in, const uint32_t* first_of, const uint32_t* rank, const uint32_t* creates,
                        const uint32_t* pl_id, K8Graph g, unsigned long long* inc);
// (7) over the sorted incidence keys: conn_pl, and conn_off at every change of node (conn_off[n_nodes] = their number)
void launch_k8_conn(hipStream_t st, const unsigned long long* inc_sorted, uint64_t n_inc, uint64_t n_nodes, K8Graph g);
// (8) 8 lanes per pair: the interval of every view both points see -> write = false: the 64-bit minimum of
//     pair * n_views + view into map[global start segment]; write = true: the claim's winner writes its record at pos[segment]
void launch_k8_iv(hipStream_t st, bool write, CloudView in, DevScene s, unsigned long long* map, const uint32_t* pos, K8Graph g);
// (9) flag[j] = map[j] is claimed, j < n_vtx; flag[n_vtx] = 0. (10) iv_off[g] = pos[pl_vtx_off[g]], g <= n_pl
void launch_k8_seg_flags(hipStream_t st, const unsigned long long* map, uint64_t n_vtx, uint32_t* flag);
void launch_k8_iv_off(hipStream_t st, DevScene s, uint32_t n_pl, const uint32_t* pos, K8Graph g);

// rocPRIM behind plain signatures (sizes are size_t: a cloud may hold more than 2^31 points). tmp == nullptr: the size query.
hipError_t k8_scan_u32(hipStream_t st, void* tmp, size_t& tmp_bytes, const uint32_t* in, uint32_t* out, size_t n);
hipError_t k8_sort_pairs(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* key_in, unsigned long long* key_out,
                         const uint32_t* val_in, uint32_t* val_out, size_t n);
hipError_t k8_sort_keys(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* key_in, unsigned long long* key_out,
                        size_t n);

}  // namespace eg3d
