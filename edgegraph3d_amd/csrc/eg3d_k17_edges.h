// Host-visible declarations of K17 (eg3d_k17_edges.hip): trace, simplify and measure the 3-D edge model of a graph3d on
// the device (include/eg3d/edges.h; the rules: eg3d_edges_core.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace eg3d {

#define K17_BLOCK 256
// the simplification: one wavefront per workgroup; a chain of at most this many vertices is staged in LDS (12 bytes each)
#define K17_LDS_VERTICES 1024
// its grid's cap: a wavefront takes chain after chain (chain, chain + grid, ...)
#define K17_SIMPLIFY_MAX_BLOCKS 8192

// flag word (ctr[K17C_FLAGS])
#define K17_FLAG_BAD_NODE 1u    // a polyline names a node outside [0, n_nodes)
#define K17_FLAG_BAD_OFFSETS 2u // conn_off does not ascend from 0 to 2 n_polylines - n_loops
#define K17_FLAG_BAD_ROW 4u     // an entry of a row: a polyline id out of range, not at that node, or twice
#define K17_FLAG_INTERNAL 8u    // a vertex would be written outside its chain (not reached on a checked graph)
enum K17Ctr { K17C_FLAGS, K17C_LOOPS, K17C_RING_HALFEDGES, K17C_RINGS, K17C_LONGEST, K17C_COUNT };

// the geometric half of a graph3d, device pointers
struct K17Graph {
  const float* node_X;
  const uint32_t* pl_start;
  const uint32_t* pl_end;
  const unsigned long long* conn_off;
  const uint32_t* conn_pl;
  uint32_t n_nodes, n_polylines;
};
// One buffer of the pointer jumping, an entry per half-edge: where the list goes on (none: its end is reached), the hops
// made so far, the smallest polyline id and the smallest from-node of the half-edges passed, and the last of them.
struct K17State {
  uint32_t *ptr, *rank, *minp, *minn, *last;
};

void launch_k17_check_polylines(hipStream_t st, K17Graph g, unsigned long long* ctr);
void launch_k17_check_offsets(hipStream_t st, K17Graph g, unsigned long long expect, unsigned long long* ctr);
void launch_k17_check_rows(hipStream_t st, K17Graph g, uint32_t* seen, uint32_t* deg, unsigned long long* ctr);
void launch_k17_successors(hipStream_t st, K17Graph g, const uint32_t* deg, uint32_t* succ, K17State s);
void launch_k17_jump(hipStream_t st, uint32_t n_halfedges, K17State in, K17State out);
void launch_k17_cut_rings(hipStream_t st, K17Graph g, const uint32_t* succ, K17State s, uint32_t* cut_node, unsigned long long* ctr);
void launch_k17_heads(hipStream_t st, K17Graph g, const uint32_t* deg, const uint32_t* cut_node, K17State s, uint32_t* head_flag,
                      uint32_t* head_of);
void launch_k17_chain_sizes(hipStream_t st, K17Graph g, const uint32_t* head_flag, const uint32_t* chain_id, const uint32_t* head_of,
                            const uint32_t* cut_node, K17State s, unsigned long long* n_vtx, uint32_t* chain_flags, uint32_t* chain_of_head,
                            unsigned long long* ctr);
void launch_k17_fill(hipStream_t st, K17Graph g, K17State s, const uint32_t* chain_of_head, const unsigned long long* chain_off,
                     uint32_t* chain_node, unsigned long long* ctr);
void launch_k17_simplify(hipStream_t st, const float* node_X, uint64_t n_chains, const unsigned long long* chain_off,
                         const uint32_t* chain_node, float maxsq, uint32_t* region, uint32_t* n_front, uint32_t* n_back,
                         unsigned long long* n_kept);
void launch_k17_compact(hipStream_t st, uint64_t n_chains, const unsigned long long* chain_off, const uint32_t* region,
                        const uint32_t* n_front, const uint32_t* n_back, const unsigned long long* s_off, uint32_t* s_node);
void launch_k17_length(hipStream_t st, const float* node_X, uint64_t n_chains, const unsigned long long* s_off, const uint32_t* s_node,
                       float* length);

}  // namespace eg3d
