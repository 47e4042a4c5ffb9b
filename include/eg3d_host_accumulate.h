/*
 * eg3d_host_accumulate.h — the PLGMatchesManager replay (row a17) as an object that lives through a run
 * (libeg3d_host.so). The reference's manager is one object: every add_matched_3dpolyline(chain) appends to the same
 * 3-D polyline graph and the same matched-interval sets, however many calls feed it. eg3d_host_replay_matches
 * (include/eg3d_host.h) builds the graph of ONE cloud; a state takes the clouds C_0 .. C_k-1 of a run one after the
 * other, and its graph is at any time, field for field and byte for byte, what eg3d_host_replay_matches builds from
 * the concatenation of the clouds added so far. The points of a cloud count from the number of points added before
 * it (node_point holds those numbers). The treatment of NaN and -1 coordinates (the reference's invalid-node wipe) is
 * the one-shot replay's, across clouds as well.
 *
 * A cloud is made of whole chains. One whose first point would continue the chain the previous cloud ended on (equal
 * key[0..2], key[3] one more) is refused, as is one that fails the checks of eg3d_host_replay_matches; a refused cloud
 * changes nothing. An empty cloud and a cloud of one-point chains add nothing (the latter's points are counted).
 */
#ifndef EG3D_HOST_ACCUMULATE_H_
#define EG3D_HOST_ACCUMULATE_H_
#include "eg3d_host.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eg3d_replay_state eg3d_replay_state;

/* `scene` is borrowed: its arrays must outlive the state. NULL: a scene without views or arrays, or out of memory. */
eg3d_replay_state* eg3d_host_replay_state_create(const eg3d_scene* scene);
/* 0, or the codes of eg3d_host_replay_matches: -1 bad arguments (a cut chain among them), -3 the points of the run
 * would reach 0xfffffff0. */
int eg3d_host_replay_state_add(eg3d_replay_state* state, const eg3d_edgepoints* pts);
/* A snapshot of the accumulated graph, released with eg3d_host_free_graph3d; the state is not disturbed. */
int eg3d_host_replay_state_graph(eg3d_replay_state* state, eg3d_graph3d* out);
/* Points of the clouds added so far: where the next cloud's points count from. */
uint64_t eg3d_host_replay_state_points(const eg3d_replay_state* state);
void eg3d_host_replay_state_destroy(eg3d_replay_state* state);

#ifdef __cplusplus
}
#endif
#endif
