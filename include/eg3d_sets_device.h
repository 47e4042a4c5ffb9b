/*
 * eg3d_sets_device.h — pipelines 1-2 with the polyline sets resident on the device, cut by polyline (libeg3d.so,
 * libeg3d_dlt4x4.so). The calls of include/eg3d.h take the "potentially compatible polylines" as host arrays and cut a
 * range into runs of WHOLE sets. Here the sets stay where K9, K11 and an upload leave them, and the unit of work is the
 * ITEM: one entry of pl_ids, i.e. one polyline of one row (set, view). The reference's output order is (set, start view,
 * polyline id, sample) — item order — so the clouds of consecutive item ranges, concatenated, are the cloud of one call.
 *
 * eg3d_device_polyline_sets is a VIEW into buffers of the context that produced it; it owns nothing. It is accepted only
 * by that context and only while it is current: each producer below states what ends that. A stale or foreign view is
 * refused with EG3D_ERR_ARG before anything of it is read.
 *
 * Producers (every id of a view has been checked against its view's polyline count before anything uses it as an index):
 *   eg3d_upload_polyline_sets          a caller's host sets. Checked ON THE DEVICE, one lane per row and one per id, after
 *                                      the upload and before the view is handed out: row_off begins at 0 and ascends, ids
 *                                      ascend strictly within a row, every id is below its view's polyline count. A
 *                                      violation returns EG3D_ERR_ARG with the texts of eg3d_match_polyline_sets. Current
 *                                      until the next eg3d_upload_polyline_sets on the context (a refused one included).
 *   eg3d_polyline_matches_device       the rows the last eg3d_match_polylines_closeness call on the context left on the
 *                                      device (K9), in place. Current until the next such call.
 *   eg3d_sets_from_communities_device  K13: compute_polyline_matches_from_nodes_component_ids on the device. The nodes
 *                                      are node_view / node_pl of the last eg3d_similarity_graph call on the context, read
 *                                      where that call left them. ids_host: the caller's ids (the file seam), or NULL for
 *                                      the ids the last eg3d_detect_communities call on the context left on the device.
 *                                      n must be that graph's n_nodes (with NULL also the node count of the community
 *                                      call). The result is eg3d_host_sets_from_communities, byte for byte: max id + 1
 *                                      sets, a node with a negative id in none, a community nobody names an empty set, a
 *                                      (view, polyline) named twice in a community counted once; EG3D_ERR_CAPACITY when
 *                                      sets x views reaches 2^32 - 1, EG3D_ERR_ARG for a wrong n, a missing graph or a
 *                                      node whose view is not one of the scene's. Current until the next call of it.
 *
 * Consumers:
 *   eg3d_polyline_item_samples   counts_host[i] = the 20 px samples of item item_begin + i (the count pass of the
 *                                extractor's sampler alone); with m, the samples left under the caller's matched
 *                                intervals. Callers and ranks balance item ranges with these and derive sample_base.
 *   eg3d_match_polyline_items    the extractor on items [item_begin, item_end): the slice of the whole-range cloud that
 *                                belongs to these items. key[0] of a point is its sample's index within the range plus
 *                                call->sample_base, so adjacent ranges, each given the samples before it as sample_base,
 *                                concatenate to the bytes of one call (obs_off rebased by the caller, as for any two
 *                                clouds). Inside the call the units are item ranges cut by the sample counts — one count
 *                                pass, a scan, the prefix sums read back — of at most EG3D_ITEM_UNIT_SAMPLES samples
 *                                (environment, read at eg3d_create; default 262 144, 32 768 from 64 views): a set larger
 *                                than a unit is cut inside it, only a single polyline stays whole. eg3d_set_pipelining
 *                                applies as to eg3d_match_polyline_sets, and every form (lanes, units, device_only)
 *                                gives the same bytes. m, device_only, out, times: as eg3d_match_polyline_sets_matched.
 *                                A unit's 32-bit totals (samples x views, epipolar hits, hypotheses) are all known before
 *                                its first chain is followed; a unit in which one wraps is cut in two by its samples and
 *                                redone, down to one item, with the same bytes. Only a single polyline that wraps on its
 *                                own returns EG3D_ERR_CAPACITY.
 *   eg3d_polyline_items_units    the number of units the last eg3d_match_polyline_items call on the context ran, and how
 *                                many times one of them was cut in two and redone.
 */
#ifndef EG3D_SETS_DEVICE_H_
#define EG3D_SETS_DEVICE_H_
#include "eg3d.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eg3d_device_polyline_sets {
  uint32_t struct_size;    /* sizeof(eg3d_device_polyline_sets), set by the producer */
  uint32_t n_sets;
  int32_t n_views;
  int32_t device;          /* HIP device the arrays live on */
  uint64_t n_ids;          /* items: entries of pl_ids = row_off[n_sets * n_views] */
  const uint32_t* row_off; /* device, [n_sets * n_views + 1] */
  const uint32_t* pl_ids;  /* device, [n_ids] */
} eg3d_device_polyline_sets;

typedef struct eg3d_items_call {
  uint32_t struct_size; /* sizeof(eg3d_items_call), set by the caller */
  uint32_t item_begin;
  uint32_t item_end;
  uint32_t sample_base; /* samples of the items before item_begin that the caller's cloud holds */
} eg3d_items_call;

typedef struct eg3d_sets_device_stats {
  uint32_t struct_size; /* sizeof(eg3d_sets_device_stats), set by the caller */
  uint32_t n_nodes;
  uint32_t n_named;     /* nodes with an id >= 0 */
  uint32_t n_sets;
  uint64_t n_ids;       /* distinct (set, view, polyline) */
  float ms_device;      /* the kernels, the sort and the read-backs between them */
  float ms_upload;      /* the caller's ids (0 with ids_host == NULL) */
} eg3d_sets_device_stats;

int eg3d_upload_polyline_sets(eg3d_ctx* ctx, const eg3d_polyline_sets* sets, eg3d_device_polyline_sets* out);
int eg3d_polyline_matches_device(eg3d_ctx* ctx, eg3d_device_polyline_sets* out);
int eg3d_sets_from_communities_device(eg3d_ctx* ctx, const int64_t* ids_host, uint64_t n, eg3d_device_polyline_sets* out,
                                      eg3d_sets_device_stats* stats);
int eg3d_polyline_item_samples(eg3d_ctx* ctx, const eg3d_device_polyline_sets* sets, uint32_t item_begin, uint32_t item_end,
                               const eg3d_matched_intervals* m, uint32_t* counts_host);
int eg3d_match_polyline_items(eg3d_ctx* ctx, const eg3d_device_polyline_sets* sets, const eg3d_items_call* call,
                              const eg3d_matched_intervals* m, int device_only, eg3d_edgepoints* out, eg3d_stage_times* times);
int eg3d_polyline_items_units(eg3d_ctx* ctx, uint32_t* n_units, uint32_t* n_redone);

#ifdef __cplusplus
}
#endif
#endif
