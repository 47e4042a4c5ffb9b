/*
 * eg3d_accumulate.h — the PLGMatchesManager replay (row a17) that accumulates over the calls of a run, on the device
 * (libeg3d.so, libeg3d_dlt4x4.so; K8a). The reference's manager is one object that lives through a run: every
 * add_matched_3dpolyline(chain) appends to the same 3-D polyline graph and the same matched-interval sets
 * (plg_matches_manager.cpp:99-180). eg3d_replay_device (include/eg3d.h) builds the graph of ONE cloud; the accumulator of a
 * context takes the clouds C_0 .. C_k-1 of a run in order — seed ranges, the steps of a pipeline, one pipeline after another
 * — so that a step's cloud can be dropped once its post steps are done, and the matched intervals can be handed to
 * eg3d_match_polyline_sets_matched between steps.
 *
 * The contract: the points of a cloud count from the number of points added before it (the context numbers them; there is
 * no index_base to get wrong), and whenever the graph is asked for it is, field for field and byte for byte, the graph that
 * eg3d_host_replay_matches builds from the concatenation of the clouds added so far: node ids by first point, node_X the
 * bits of that first point (-0.0 kept), node_point the run-wide number of the node's last point, polylines numbered and
 * oriented by their creating pair, conn ascending, intervals by first claim in the order (pair, view ascending). Every
 * order-dependent rule of the replay is a first-claim or last-writer rule over point numbers, so nothing an earlier cloud
 * decided is revised by a later one. Asking for the graph does not disturb the state; a call that asks for nothing
 * (out_dev == NULL and out_host == NULL) only adds its claims. The state is O(nodes + polylines + scene vertices) of HBM,
 * not O(points of the run), and goes with the context. A clone has its own accumulator, empty at first.
 *
 * cloud: as for eg3d_replay_device (NULL = the context's last device output, which must be `complete`). A cloud is made of
 * whole chains, as every cloud of an eg3d_match_* call is. An empty cloud, or one of one-point chains only, adds nothing and
 * is accepted (its points are counted). reset != 0 starts a new graph with this cloud.
 *
 * Refused, by checks that run before anything of the state is changed (the state, a reset asked for by the refused call
 * included, out_dev, out_host and stats are left as they were, and the next valid cloud continues from there):
 *   EG3D_ERR_ARG       what eg3d_replay_device refuses with it; and a chain cut between two clouds: the first point of the
 *                      cloud has the key the previous cloud's last point would continue (equal key[0..2], key[3] one more);
 *   EG3D_ERR_HOSTONLY  a NaN coordinate, or x or y == -1, in a point of a pair: accumulate such a run on the host
 *                      (include/eg3d_host_accumulate.h keeps the reference's invalid-node wipe across clouds);
 *   EG3D_ERR_CAPACITY  the points of the run would reach 0xfffffff0.
 * A HIP or allocation failure after the claims began invalidates the state: every later call without reset != 0 answers
 * EG3D_ERR_ARG and says so.
 *
 * out_dev: views the accumulator's own buffers, valid until the next eg3d_replay_accumulate on this context; its interval
 * arrays are usable in place as an eg3d_matched_intervals{on_device = 1}. eg3d_replay_device and the accumulator do not
 * disturb each other: each call invalidates the out_dev of the earlier calls of ITS OWN entry point only. out_host: a
 * library-owned copy, released with eg3d_free_graph3d. stats: the accumulated totals (n_pairs, n_nodes, n_polylines,
 * n_intervals) and the node table's size in use; ms_graph = this cloud's claims, ms_intervals = the materialisation (0
 * without out_dev and out_host), ms_copy = the copy to the host. The node table grows by rehash when the lookups of the
 * run (two per pair) ask for more than eg3d_replay_device would take for as many; EG3D_REPLAY_TABLE_BITS keeps its
 * meaning as the minimum.
 */
#ifndef EG3D_ACCUMULATE_H_
#define EG3D_ACCUMULATE_H_
#include "eg3d.h"

#ifdef __cplusplus
extern "C" {
#endif

int eg3d_replay_accumulate(eg3d_ctx* ctx, const eg3d_device_edgepoints* cloud, int reset, eg3d_device_graph3d* out_dev,
                           struct eg3d_graph3d* out_host, eg3d_replay_stats* stats);
/* The running totals (any pointer may be NULL): n_points is what eg3d_dedup_device wants as index_base for the next cloud
 * of the run; state_bytes the HBM the state holds (the scratch of a call and the materialised graph not counted). */
int eg3d_replay_accumulated(eg3d_ctx* ctx, uint64_t* n_points, uint64_t* n_pairs, uint64_t* state_bytes);

#ifdef __cplusplus
}
#endif
#endif
