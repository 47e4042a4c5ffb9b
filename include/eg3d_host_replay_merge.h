/*
 * eg3d_host_replay_merge.h — the matches manager (row a17) joins the GRAPH of the run that follows, on the host
 * (libeg3d_host.so). A state of include/eg3d_host_accumulate.h takes the clouds of a run in order; this entry point lets
 * it take, in place of a cloud, the graph that a replay of that cloud built somewhere else — another state, another
 * process, a GPU — so that shards of a run are replayed apart and only their graphs travel. Every order-dependent rule of
 * the replay is a first-claim or a last-writer rule over point numbers, so the graph of "A followed directly by B" follows
 * from the graph of A, the number of points of A and the graph of B alone:
 *
 *   nodes      B's nodes in B's id order (= the order of their first points). One whose canonical coordinates (bit
 *              patterns, -0 counted as +0) are a node of A IS that node: node_X stays A's bits, node_point becomes
 *              nA + B.node_point. Any other is new: id = A's node count + its rank among B's new nodes, node_X = B's bits
 *              as stored, node_point rebased by nA.
 *   polylines  B's polylines in B's id order, endpoints mapped. One whose unordered node pair A holds is A's polyline (id
 *              and orientation unchanged). Any other is new: id = A's polyline count + its rank among the new ones, in
 *              B's orientation; loops are allowed. conn is derived when the graph is asked for, as ever.
 *   intervals  a cell is (scene polyline, start segment). A cell claimed in A keeps A's record; one claimed only in B
 *              takes B's. Within a scene polyline the records are ordered by start segment.
 *   points     the run now has nA + nB points.
 *
 * `later` must be the graph of the run that follows DIRECTLY and of whole chains (seed ranges are). Merging is associative
 * over adjacent runs: a fold in shard order and a pairwise tree give the same bytes, and both give what
 * eg3d_host_replay_matches builds from the concatenation of all clouds. Merging into an empty state yields `later`
 * itself. A graph does not carry the key its cloud ended on, so the cut-chain check of eg3d_host_replay_state_add is
 * skipped for the first cloud added after a merge.
 *
 * Only n_nodes, n_real_nodes, node_X, node_point, n_polylines, pl_start, pl_end, n_scene_polylines and the iv_* arrays of
 * `later` are read (conn_* may be NULL). Returns 0, or — the state is then as it was —
 *   -1  null arguments; n_scene_polylines differs from the scene's; an endpoint >= n_nodes; a node_point >= later_points
 *       (so a graph with more nodes or polylines than points); iv_off that does not begin at 0, does not ascend or gives a
 *       scene polyline more intervals than it has segments; a start or end segment outside its scene polyline; start
 *       segments within a scene polyline that do not ascend strictly; two nodes of `later` with equal canonical
 *       coordinates; two polylines of `later` on one unordered node pair;
 *   -3  the points of the run would reach 0xfffffff0;
 *   -5  the state or `later` holds wiped or invalid nodes (n_real_nodes != n_nodes; a NaN, or an x or y equal to -1, in
 *       node_X): the rule above does not cover the reference's invalid-node wipe. Add such a run's clouds instead.
 * -1 takes precedence over -5.
 */
#ifndef EG3D_HOST_REPLAY_MERGE_H_
#define EG3D_HOST_REPLAY_MERGE_H_
#include "eg3d_host_accumulate.h"

#ifdef __cplusplus
extern "C" {
#endif

int eg3d_host_replay_state_merge_graph(eg3d_replay_state* state, const eg3d_graph3d* later, uint64_t later_points);

#ifdef __cplusplus
}
#endif
#endif
