/*
 * eg3d_replay_merge.h — the matches manager (row a17) joins the GRAPH of the run that follows, on the device (libeg3d.so,
 * libeg3d_dlt4x4.so; K8m). eg3d_replay_accumulate (include/eg3d_accumulate.h) needs the clouds of a run to pass through one
 * context in order. Here the accumulator of a context takes, in place of a cloud, the graph that a replay of that cloud
 * built on another context — a clone or lane on this device, another rank whose arrays were gathered — so that the shards
 * of a run are replayed apart and only their graphs travel: 12 + 8 bytes per node, 8 per polyline and at most one interval
 * per scene vertex, no observation lists. The rule is stated in include/eg3d_host_replay_merge.h; csrc/eg3d_k8m_merge.hip
 * states it in kernels.
 *
 * The contract: after any mixture of eg3d_replay_accumulate (clouds) and eg3d_replay_merge_graph (graphs) in run order the
 * accumulated graph is, field for field and byte for byte, what eg3d_host_replay_matches builds from the concatenation of
 * all clouds of the run. `later` must be the graph of the run that follows DIRECTLY and of whole chains. Merging is
 * associative over adjacent runs, so a fold in shard order and a pairwise tree give the same bytes. Merging into an empty
 * or reset accumulator yields `later` itself. eg3d_replay_accumulated reports the summed points and pairs.
 *
 * later: its arrays are device-readable on ctx's device and final when the call is made: the out_dev of ANOTHER context's
 * eg3d_replay_device or eg3d_replay_accumulate on that device, or uploaded arrays. Only n_nodes, n_real_nodes, node_X,
 * node_point, n_polylines, pl_start, pl_end, n_scene_polylines and the iv_* arrays are read; conn_* may be NULL.
 * later_points: the points of the cloud `later` was built from. later_pairs: only added to the totals (the n_pairs of the
 * stats of the replay that built `later`). reset, out_dev, out_host, stats: as for eg3d_replay_accumulate — the
 * accumulated totals, ms_graph = this call's claims, ms_intervals = the materialisation, ms_copy.
 *
 * A graph does not carry the key its cloud ended on, so the cut-chain check of eg3d_replay_accumulate is skipped for the
 * first cloud accumulated after a merge. The node table grows by rehash as needed (it keeps more than twice as many slots
 * as the state has nodes); EG3D_REPLAY_TABLE_BITS keeps its meaning as the minimum.
 *
 * Refused, by checks that run on the device before anything of `later` is used as an index and before anything of the
 * state changes (the state, a reset asked for by the refused call included, out_dev, out_host and stats are left as they
 * were, and a refused graph causes no access outside its arrays):
 *   EG3D_ERR_ARG       null arguments; n_scene_polylines differs from the scene's; an endpoint >= n_nodes; a node_point >=
 *                      later_points (so a graph with more nodes or polylines than points); iv_off that does not begin at 0,
 *                      does not ascend or gives a scene polyline more intervals than it has segments (an invalid polyline
 *                      has none); a start or end segment outside its scene polyline; start segments within a scene
 *                      polyline that do not ascend strictly; two nodes of `later` with equal canonical coordinates (a
 *                      -0 / +0 pair counts); two polylines of `later` on one unordered node pair; `later` aliasing this
 *                      accumulator's own out_dev; a state invalidated by an earlier failure (without reset);
 *   EG3D_ERR_HOSTONLY  n_real_nodes != n_nodes; a NaN, or an x or y equal to -1, in node_X (the host form refuses these
 *                      too: add such a run's clouds to a host state instead);
 *   EG3D_ERR_CAPACITY  the points of the run would reach 0xfffffff0 (judged from later_points alone, before any launch).
 * EG3D_ERR_ARG takes precedence over EG3D_ERR_HOSTONLY.
 */
#ifndef EG3D_REPLAY_MERGE_H_
#define EG3D_REPLAY_MERGE_H_
#include "eg3d_accumulate.h"

#ifdef __cplusplus
extern "C" {
#endif

int eg3d_replay_merge_graph(eg3d_ctx* ctx, const eg3d_device_graph3d* later, uint64_t later_points, uint64_t later_pairs,
                            int reset, eg3d_device_graph3d* out_dev, struct eg3d_graph3d* out_host,
                            eg3d_replay_stats* stats);

#ifdef __cplusplus
}
#endif
#endif
