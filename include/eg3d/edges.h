/*
 * eg3d/edges.h — trace, simplify and measure the 3-D edge model of the matched graph where it lies, K17 (libeg3d.so,
 * libeg3d_dlt4x4.so; the result does not depend on the DLT form). The rules are those of include/eg3d/host_edges.h, the
 * bytes those of eg3d_host_edge_chains on a host copy of the same graph: only the simplified model has to travel.
 *
 * On the device the trace ranks the half-edges (polyline, side) by pointer jumping — ceil(log2(2 n_polylines)) rounds, a
 * number the host computes; what has reached no end after them lies on a ring, which is cut at its smallest node id and
 * ranked again — and numbers the chains by a scan of their smallest polyline ids. The simplification runs one wavefront
 * per chain, the lanes splitting the interior points of each linearizable_polyline test and combining with a ballot
 * ("any distance > maxsq": a predicate, so the result is that of the sequential test). The length is one lane per chain,
 * a sequential FP32 sum in vertex order.
 *
 * Refused with EG3D_ERR_ARG before anything is indexed, `out_dev`, `out_host`, `stats` and an earlier result of the context
 * untouched: what include/eg3d/host_edges.h lists (the checks run on the device), a null context, a stats struct smaller
 * than the library's, g == NULL on a context without a replay result. EG3D_ERR_CAPACITY: 2^30 nodes or polylines.
 */
#ifndef EG3D_EDGES_H_
#define EG3D_EDGES_H_
#include "../eg3d.h"
#include "host_edges.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eg3d_device_edge_chains { /* the members of eg3d_edge_chain_set, the pointers into HBM */
  uint64_t n_chains;
  uint64_t n_vertices;
  uint64_t n_kept;
  const uint64_t* chain_off;
  const uint32_t* chain_node;
  const uint32_t* chain_flags;
  const uint64_t* s_off;
  const uint32_t* s_node;
  const float* length;
} eg3d_device_edge_chains;

/* g: any graph on ctx's device (eg3d_replay_device, eg3d_replay_accumulate, eg3d_replay_merge_graph, caller-built), read in
 * place; NULL = the result of the context's last eg3d_replay_device. out_dev: buffers of the context that are separate
 * from the match, compaction and replay buffers, valid until the next call of either entry point on this context.
 * out_host: a library-owned copy, released with eg3d_free_edge_chains. Any of out_dev, out_host, stats may be NULL. */
int eg3d_edge_chains_device(eg3d_ctx* ctx, const eg3d_device_graph3d* g, float max_dist, int simplify,
                            eg3d_device_edge_chains* out_dev, eg3d_edge_chain_set* out_host, eg3d_edges_stats* stats);

/* the same on a host graph, uploaded for the call (ms_copy includes the upload) */
int eg3d_edge_chains(eg3d_ctx* ctx, const eg3d_graph3d* host_graph, float max_dist, int simplify,
                     eg3d_device_edge_chains* out_dev, eg3d_edge_chain_set* out_host, eg3d_edges_stats* stats);

void eg3d_free_edge_chains(eg3d_edge_chain_set* chains);

#ifdef __cplusplus
}
#endif
#endif
