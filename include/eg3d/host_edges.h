/*
 * eg3d/host_edges.h — the 3-D edge model of the matched graph, its sequential statement (libeg3d_host.so).
 *
 * The graph the PLGMatchesManager replay builds (eg3d_graph3d, include/eg3d_host.h) holds one 2-node polyline per direct
 * connection of two edge-points. This turns it into line geometry with the operations the reference's PolyLineGraph3D has
 * for that (plgs/polyline_graph_3d.cpp: simplify_polyline :147-250, update_length :57-61, get_segments_list :133-141, and
 * the meeting of two polylines in a node that merge_polylines :298-353 joins):
 *
 *   trace     the graph's non-loop polylines joined into maximal CHAINS through the nodes of degree 2; a chain is open
 *             (it ends in nodes of another degree) or a ring. Chains are numbered by their smallest polyline id; an open
 *             chain starts at the end whose end polyline has the smaller id (one polyline: pl_start -> pl_end), a ring at
 *             its smallest node id along the smaller of that node's two polyline ids, the start node repeated at the end.
 *             A loop (pl_start == pl_end) is in no chain and in no degree; a node of degree 0 is in no chain.
 *   simplify  simplify_polyline on every chain's vertices with the tolerance max_dist (scene units; the reference's 3-D
 *             constant is 0.01, polyline_graph_3d.hpp:65 — no default suits every scene), FP32 in glm's evaluation order.
 *             E1: a chain whose first and last vertex are the same node is simplified without its last vertex, which is
 *             appended again (the reference's rule would collapse it to two equal points: every distance to a line of
 *             direction 0 is NaN, and NaN > maxsq is false).
 *   length    update_length on the kept vertices: an FP32 sum in vertex order.
 * csrc/eg3d_edges_core.h is the statement; eg3d_edge_chains_device (include/eg3d/edges.h) computes the same bytes on the
 * device.
 *
 * Only n_nodes, node_X, n_polylines, pl_start, pl_end, conn_off and conn_pl of the graph are read. It is checked before
 * anything is indexed with it; a failure returns EG3D_ERR_ARG (-1) and leaves `out` and `stats` untouched:
 *   node ids and polyline ids in range; conn_off ascending from 0 and ending at the table's length; no polyline twice in
 *   a row; every entry of a row names a polyline that has that node as an end; the table holds
 *   2 * n_polylines - n_loops entries; max_dist finite and >= 0; n_nodes and n_polylines below 2^30 (-3 otherwise).
 */
#ifndef EG3D_HOST_EDGES_H_
#define EG3D_HOST_EDGES_H_
#include "../eg3d_host.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EG3D_EDGES_FLAG_RING 1u

/* (the type is a chain SET: eg3d_edge_chains and eg3d_host_edge_chains are the functions, and C keeps typedef names and
 * function names in one name space) */
typedef struct eg3d_edge_chain_set {
  uint64_t n_chains;
  uint64_t n_vertices;    /* = chain_off[n_chains] */
  uint64_t n_kept;        /* = s_off[n_chains] */
  uint64_t* chain_off;    /* [n_chains + 1] */
  uint32_t* chain_node;   /* [n_vertices] node ids, chain after chain in vertex order */
  uint32_t* chain_flags;  /* [n_chains] EG3D_EDGES_FLAG_RING */
  uint64_t* s_off;        /* [n_chains + 1] the kept vertices ... */
  uint32_t* s_node;       /* [n_kept] ... as node ids (node_X, node_point of the graph still apply) */
  float* length;          /* [n_chains] of the kept polyline */
} eg3d_edge_chain_set;

typedef struct eg3d_edges_stats {
  uint32_t struct_size;   /* sizeof(eg3d_edges_stats), set by the caller; a smaller value is refused */
  uint32_t reserved;
  uint64_t n_chains;
  uint64_t n_rings;
  uint64_t n_loops_dropped;
  uint64_t n_vertices_in;
  uint64_t n_vertices_kept;
  uint64_t longest_chain;  /* vertices of the longest traced chain */
  float ms_trace;
  float ms_simplify;
  float ms_copy;
  float reserved2;
} eg3d_edges_stats;

/* simplify == 0: the traced chains unsimplified (s_off / s_node repeat chain_off / chain_node; max_dist is still checked).
 * stats may be NULL; the times of the host form are wall times (ms_copy 0). */
int eg3d_host_edge_chains(const eg3d_graph3d* graph, float max_dist, int simplify, eg3d_edge_chain_set* out, eg3d_edges_stats* stats);
void eg3d_host_free_edge_chains(eg3d_edge_chain_set* chains);

/* An ASCII PLY line model: one `element vertex` per distinct kept node, ascending node id, renumbered from 0; one
 * `element edge` (vertex1, vertex2) per consecutive kept pair, in chain order — the segment list of get_segments_list.
 * Coordinates are written as eg3d_host_write_ply writes them (%g of the widened value). node_X: [.][3], indexed by the
 * chains' node ids. Returns 0, -1 (arguments), -2 (the file). */
int eg3d_host_write_ply_edges(const char* path, const eg3d_edge_chain_set* chains, const float* node_X);

#ifdef __cplusplus
}
#endif
#endif
