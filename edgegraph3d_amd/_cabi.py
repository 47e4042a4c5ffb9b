"""The C ABI as ctypes sees it: one hand-written table per public header, function name -> (restype, argtypes), and HEADERS,
which says which library carries each table; bind_library() declares all of a library's tables on a CDLL. tests/test_abi.py
reads every header of include/ and holds every row, every struct mirror (_cdefs.MIRRORS) and every built library to them.
The next header: write it, add its table and one HEADERS row here and the mirrors of its structs to _cdefs.MIRRORS.
eg3d.h, eg3d_host.h and eg3d_rccl.h are frozen: a new entry point gets a header of its own."""
import ctypes as C

from . import _cdefs as D

P = C.POINTER
vp, cstr, i32, u32, i64p = C.c_void_p, C.c_char_p, C.c_int, C.c_uint32, P(C.c_int64)
u64, f32, intp = C.c_uint64, C.c_float, P(C.c_int)
f32p, f64p, u8p, u32p, i32p, u64p = D.f32p, D.f64p, D.u8p, D.u32p, D.i32p, D.u64p

# include/eg3d.h (libeg3d.so, libeg3d_dlt4x4.so); a context handle (eg3d_ctx*) is a void pointer here
EG3D = {
    "eg3d_last_error": (cstr, []),
    "eg3d_device_count": (i32, []),
    "eg3d_dlt_rows": (i32, []),
    "eg3d_create": (i32, [P(D.Scene), i32, P(vp)]),
    "eg3d_destroy": (None, [vp]),
    "eg3d_clone": (i32, [vp, P(vp)]),
    "eg3d_get_grid": (i32, [vp, i32, i32, u32p, u32p, P(u32p), P(u32p)]),
    "eg3d_candidates_run": (i32, [vp, P(D.Seeds), u32, u32, P(D.Candidates)]),
    "eg3d_free_candidates": (None, [P(D.Candidates)]),
    "eg3d_match_refpoints": (i32, [vp, P(D.Seeds), u32, u32, i32, P(D.EdgePoints), P(D.StageTimes)]),
    "eg3d_match_polyline_sets": (i32, [vp, P(D.PolylineSets), u32, u32, i32, P(D.EdgePoints), P(D.StageTimes)]),
    "eg3d_match_polyline_sets_matched": (i32, [vp, P(D.PolylineSets), u32, u32, P(D.MatchedIntervals), i32, P(D.EdgePoints),
                                               P(D.StageTimes)]),
    "eg3d_polyline_set_candidates": (i32, [vp, P(D.PolylineSets), u32, u32, P(D.MatchedIntervals), P(D.SetCandidates)]),
    "eg3d_free_set_candidates": (None, [P(D.SetCandidates)]),
    "eg3d_check_polyline_sets": (i32, [P(D.PolylineSets), C.c_int32]),
    "eg3d_free_edgepoints": (None, [P(D.EdgePoints)]),
    "eg3d_upload_seeds": (i32, [vp, P(D.Seeds)]),
    "eg3d_match_resident": (i32, [vp, u32, u32, i32, P(D.EdgePoints), P(D.StageTimes)]),
    "eg3d_set_pipelining": (i32, [vp, i32, i32]),
    "eg3d_last_device_output": (i32, [vp, P(D.DeviceEdgePoints)]),
    "eg3d_gn_filter": (i32, [vp, f32p, u32p, i32p, f32p, u64, f32, i32, f32p, u8p, f32p]),
    "eg3d_context_info": (i32, [vp, P(C.c_int32), P(C.c_int32)]),
    "eg3d_gn_filter_device": (i32, [vp, P(D.DeviceEdgePoints), vp, f32, i32, vp, vp, u64p, u64p, f32p]),
    "eg3d_compact_device": (i32, [vp, P(D.DeviceEdgePoints), vp, vp, C.c_int32, P(D.DeviceEdgePoints)]),
    "eg3d_filter_resident": (i32, [vp, f32, i32, i32, u64p, i32, P(D.EdgePoints), P(D.DeviceEdgePoints), P(D.FilterStats)]),
    "eg3d_dedup_device": (i32, [vp, P(D.DeviceEdgePoints), u64, i32, vp, u64p]),
    "eg3d_dedup_resident": (i32, [vp, u64, i32, i32, f32, i32, i32, u64p, i32, P(D.EdgePoints), P(D.DeviceEdgePoints),
                                  P(D.DedupStats)]),
    "eg3d_replay_device": (i32, [vp, P(D.DeviceEdgePoints), P(D.DeviceGraph3D), P(D.Graph3D), P(D.ReplayStats)]),
    "eg3d_free_graph3d": (None, [P(D.Graph3D)]),
    "eg3d_match_polylines_closeness": (i32, [vp, P(D.Seeds), u32, u32, P(D.PolylineMatches), P(D.PolymatchStats)]),
    "eg3d_free_polyline_matches": (None, [P(D.PolylineMatches)]),
    "eg3d_similarity_graph": (i32, [vp, P(D.Seeds), u32, u32, P(D.Simgraph), P(D.SimgraphStats)]),
    "eg3d_free_simgraph": (None, [P(D.Simgraph)]),
    "eg3d_detect_communities": (i32, [vp, P(D.Simgraph), P(D.LouvainParams), P(D.Communities), P(D.LouvainStats)]),
    "eg3d_free_communities": (None, [P(D.Communities)]),
    "eg3d_estimate_fundamental": (i32, [i32, C.c_int32, P(D.Seeds), P(D.FundParams), f64p, u8p, u32p, P(D.FundStats)]),
}

# include/eg3d_host.h (libeg3d_host.so); the eg3d_synth*, eg3d_plg* and eg3d_sfm* handles are void pointers here
EG3D_HOST = {
    "eg3d_synth_default_config": (None, [P(D.SynthConfig), i32]),
    "eg3d_synth_create": (vp, [P(D.SynthConfig)]),
    "eg3d_synth_scene": (P(D.Scene), [vp]),
    "eg3d_synth_seeds": (P(D.Seeds), [vp]),
    "eg3d_synth_seed_truth": (f32p, [vp]),
    "eg3d_synth_total_segments": (u64, [vp]),
    "eg3d_synth_polyline_curve": (u32p, [vp]),
    "eg3d_synth_n_curves": (i32, [vp]),
    "eg3d_synth_destroy": (None, [vp]),
    "eg3d_synth_points": (i32, [vp, u64, u64, P(f32p), P(u32p), P(i32p), P(f32p)]),
    "eg3d_host_free": (None, [vp]),
    "eg3d_synth_camera": (i32, [vp, i32, f32p, f32p, f32p, f32p, f32p]),
    "eg3d_plg_write": (i32, [cstr, P(D.Scene)]),
    "eg3d_plg_read": (vp, [cstr]),
    "eg3d_plg_scene": (P(D.Scene), [vp]),
    "eg3d_plg_destroy": (None, [vp]),
    "eg3d_plg_build_from_mask": (i32, [u8p, i32, i32, P(D.PlgView)]),
    "eg3d_png_read_edge_mask": (i32, [cstr, intp, intp, P(u8p)]),
    "eg3d_plg_build_from_png": (i32, [cstr, intp, intp, P(D.PlgView)]),
    "eg3d_plg_view_free": (None, [P(D.PlgView)]),
    "eg3d_plg_build_views_from_png": (i32, [P(cstr), i32, intp, intp, P(D.PlgView)]),
    "eg3d_plg_from_views": (vp, [i32, i32, i32, P(D.PlgView)]),
    "eg3d_host_build_grid": (i32, [P(D.Scene), i32, f32, u32p, u32p, P(u32p), P(u32p), u32p]),
    "eg3d_host_filter_close_2d": (i32, [i32, i32, i32, P(D.EdgePoints), u8p]),
    "eg3d_host_observation_filter": (i32, [i32, u32p, u64, u64, i32, u8p]),
    "eg3d_host_gather_plan": (i32, [i32, u64p, u64p, u64p, u64p, u64p]),
    "eg3d_host_gather_place": (i32, [P(D.EdgePoints), u64, u64, P(D.EdgePoints)]),
    "eg3d_host_replay_matches": (i32, [P(D.Scene), P(D.EdgePoints), P(D.Graph3D)]),
    "eg3d_host_free_graph3d": (None, [P(D.Graph3D)]),
    "eg3d_host_is_matched": (i32, [P(D.Scene), P(D.MatchedIntervals), u64, i32p, u32p, u32p, f32p, i64p]),
    "eg3d_host_write_compat_graph": (i32, [cstr, P(D.Simgraph)]),
    "eg3d_host_read_communities": (i32, [cstr, P(i64p), u64p]),
    "eg3d_host_write_communities": (i32, [cstr, i64p, u64]),
    "eg3d_host_sets_from_communities": (i32, [P(D.Simgraph), i64p, u64, C.c_int32, P(D.PolylineSets)]),
    "eg3d_host_free_polyline_sets": (None, [P(D.PolylineSets)]),
    "eg3d_sfm_read_json": (vp, [cstr]),
    "eg3d_sfm_write_json": (i32, [vp, cstr, cstr]),
    "eg3d_host_camera_model": (i32, [u64, f32p, f32p, f32p, f32p, f32p]),
    "eg3d_host_json_double_text": (i32, [C.c_double, cstr, i32]),
    "eg3d_host_json_number_text": (i32, [cstr, cstr, i32]),
    "eg3d_host_json_cached_power": (i32, [i32, u64p, intp]),
    "eg3d_sfm_create": (vp, [i32, i32, i32]),
    "eg3d_sfm_destroy": (None, [vp]),
    "eg3d_sfm_n_views": (i32, [vp]),
    "eg3d_sfm_n_points": (u64, [vp]),
    "eg3d_sfm_cam_P": (f32p, [vp]),
    "eg3d_sfm_image_path": (cstr, [vp, i32]),
    "eg3d_sfm_image_size": (i32, [vp, intp, intp]),
    "eg3d_sfm_set_camera": (i32, [vp, i32, f32, f32, f32, f32p, f32p, cstr]),
    "eg3d_sfm_seeds": (i32, [vp, P(D.Seeds)]),
    "eg3d_sfm_points": (f32p, [vp]),
    "eg3d_sfm_add_point": (i32, [vp, f32p, i32, i32p, f32p]),
    "eg3d_sfm_add_edgepoints": (i32, [vp, P(D.EdgePoints), u8p]),
    "eg3d_sfm_remove_outliers": (i32, [vp, u8p]),
    "eg3d_sfm_set_point_coords": (i32, [vp, f32p]),
    "eg3d_sfm_analytic_F": (i32, [vp, f64p, u8p]),
    "eg3d_host_estimate_F": (i32, [i32, u64, u32p, i32p, f32p, i32, u64, f64p, u8p, u32p]),
    "eg3d_sfm_estimate_F": (i32, [vp, i32, u64, f64p, u8p, u32p]),
    "eg3d_host_estimate_fundamental": (i32, [C.c_int32, P(D.Seeds), P(D.FundParams), f64p, u8p, u32p, P(D.FundStats)]),
}

# include/eg3d_rccl.h (libeg3d_rccl.so); communicator, gather handle and stream are void pointers here
EG3D_RCCL = {
    "eg3d_comm_unique_id": (i32, [vp]),
    "eg3d_comm_init": (i32, [vp, i32, i32, i32, P(vp)]),
    "eg3d_comm_query": (i32, [vp, intp, intp, intp]),
    "eg3d_comm_destroy": (None, [vp]),
    "eg3d_gather_create": (vp, [i32]),
    "eg3d_gather_destroy": (None, [vp]),
    "eg3d_gather_set_mode": (i32, [vp, i32]),
    "eg3d_gather_set_chunk_bytes": (i32, [vp, u64]),
    "eg3d_allgather_edgepoints": (i32, [vp, vp, i32, i32, vp, P(D.DeviceEdgePoints), P(D.DeviceEdgePoints), u64p, u64p]),
    "eg3d_concat_edgepoints": (i32, [vp, i32, P(D.DeviceEdgePoints), vp, P(D.DeviceEdgePoints)]),
}

# include/eg3d_accumulate.h (libeg3d.so, libeg3d_dlt4x4.so): the replay that accumulates over the calls of a run
EG3D_ACCUMULATE = {
    "eg3d_replay_accumulate": (i32, [vp, P(D.DeviceEdgePoints), i32, P(D.DeviceGraph3D), P(D.Graph3D), P(D.ReplayStats)]),
    "eg3d_replay_accumulated": (i32, [vp, u64p, u64p, u64p]),
}

# include/eg3d_host_accumulate.h (libeg3d_host.so); the eg3d_replay_state handle is a void pointer here
EG3D_HOST_ACCUMULATE = {
    "eg3d_host_replay_state_create": (vp, [P(D.Scene)]),
    "eg3d_host_replay_state_add": (i32, [vp, P(D.EdgePoints)]),
    "eg3d_host_replay_state_graph": (i32, [vp, P(D.Graph3D)]),
    "eg3d_host_replay_state_points": (u64, [vp]),
    "eg3d_host_replay_state_destroy": (None, [vp]),
}

# include/eg3d_dedup_phases.h (libeg3d.so, libeg3d_dlt4x4.so): the 3 px dedup as claim / keep / the map / the merge of maps
EG3D_DEDUP_PHASES = {
    "eg3d_dedup_claim": (i32, [vp, P(D.DeviceEdgePoints), u64, i32]),
    "eg3d_dedup_keep": (i32, [vp, P(D.DeviceEdgePoints), u64, vp, u64p]),
    "eg3d_dedup_claims": (i32, [vp, P(vp), u64p]),
    "eg3d_dedup_merge_claims": (i32, [vp, vp, u64, u64p]),
    "eg3d_dedup_phase_ms": (i32, [vp, f32p]),
}

# include/eg3d_host_dedup_phases.h (libeg3d_host.so): their sequential definition on host clouds
EG3D_HOST_DEDUP_PHASES = {
    "eg3d_host_dedup_n_cells": (u64, [i32, i32, i32]),
    "eg3d_host_dedup_claim": (i32, [i32, i32, i32, P(D.EdgePoints), u64, u32p]),
    "eg3d_host_dedup_keep": (i32, [i32, i32, i32, P(D.EdgePoints), u64, u32p, u8p, u64p]),
    "eg3d_host_dedup_merge": (i32, [u32p, u32p, u64]),
}

# include/eg3d_rccl_claims.h (libeg3d_rccl.so): the minimum all-reduce of the claim maps and the scan of the point counts
EG3D_RCCL_CLAIMS = {
    "eg3d_allreduce_claims": (i32, [vp, i32, i32, vp, vp, u64, i32, u64]),
    "eg3d_exscan_points": (i32, [vp, i32, i32, vp, u64, u64p, u64p]),
}

# include/eg3d_replay_merge.h (libeg3d.so, libeg3d_dlt4x4.so): the accumulator takes the graph of the run that follows
EG3D_REPLAY_MERGE = {
    "eg3d_replay_merge_graph": (i32, [vp, P(D.DeviceGraph3D), u64, u64, i32, P(D.DeviceGraph3D), P(D.Graph3D), P(D.ReplayStats)]),
}

# include/eg3d_host_replay_merge.h (libeg3d_host.so): its sequential definition on a host state
EG3D_HOST_REPLAY_MERGE = {
    "eg3d_host_replay_state_merge_graph": (i32, [vp, P(D.Graph3D), u64]),
}

# include/eg3d_sets_device.h (libeg3d.so, libeg3d_dlt4x4.so): polyline sets resident on the device, the extractor on item
# ranges
EG3D_SETS_DEVICE = {
    "eg3d_upload_polyline_sets": (i32, [vp, P(D.PolylineSets), P(D.DevicePolylineSets)]),
    "eg3d_polyline_matches_device": (i32, [vp, P(D.DevicePolylineSets)]),
    "eg3d_sets_from_communities_device": (i32, [vp, i64p, u64, P(D.DevicePolylineSets), P(D.SetsDeviceStats)]),
    "eg3d_polyline_item_samples": (i32, [vp, P(D.DevicePolylineSets), u32, u32, P(D.MatchedIntervals), u32p]),
    "eg3d_match_polyline_items": (i32, [vp, P(D.DevicePolylineSets), P(D.ItemsCall), P(D.MatchedIntervals), i32, P(D.EdgePoints),
                                        P(D.StageTimes)]),
    "eg3d_polyline_items_units": (i32, [vp, u32p, u32p]),
}

# include/eg3d_triangulate.h (libeg3d.so, libeg3d_dlt4x4.so): FP64 triangulation of caller-supplied tracks, K14
EG3D_TRIANGULATE = {
    "eg3d_triangulate": (i32, [vp, i32, u64, u32p, i32p, f32p, f32p, f32p, u8p, u8p, P(D.TriStats)]),
    "eg3d_triangulate_device": (i32, [vp, i32, P(D.DeviceEdgePoints), vp, vp, vp, P(D.TriStats)]),
}

# include/eg3d_host_triangulate.h (libeg3d_host.so): its sequential statement, both DLT forms
EG3D_HOST_TRIANGULATE = {
    "eg3d_host_triangulate": (i32, [i32, f32p, i32, i32, u64, u32p, i32p, f32p, f32p, i32, f32p, u8p, u8p]),
}

# include/eg3d_colour.h (libeg3d.so, libeg3d_dlt4x4.so): the colours of a cloud from the source images, K15
EG3D_COLOUR = {
    "eg3d_upload_images": (i32, [vp, i32, i32p, i32p, P(u8p)]),
    "eg3d_release_images": (i32, [vp]),
    "eg3d_colour_device": (i32, [vp, P(D.DeviceEdgePoints), vp, vp, vp, P(D.ColourStats)]),
    "eg3d_colour_points": (i32, [vp, u64, u32p, i32p, f32p, u8p, u8p, u8p, P(D.ColourStats)]),
}

# include/eg3d_host_colour.h (libeg3d_host.so): its sequential statement, the PLY writer, the RGB PNG reader
EG3D_HOST_COLOUR = {
    "eg3d_host_colour_points": (i32, [i32, i32p, i32p, P(u8p), u64, u32p, i32p, f32p, u8p, i32, u8p, u8p, u64p]),
    "eg3d_host_reflect101_loop": (i32, [i32, i32]),
    "eg3d_host_reflect101_closed": (i32, [i32, i32]),
    "eg3d_host_write_ply": (i32, [cstr, u64, f32p, u8p, u8p]),
    "eg3d_host_png_read_rgb": (i32, [cstr, intp, intp, P(u8p)]),
}

# include/eg3d_transform.h (libeg3d.so, libeg3d_dlt4x4.so): a 4 x 4 transform applied to a cloud's points, K16
EG3D_TRANSFORM = {
    "eg3d_transform_device": (i32, [vp, P(D.DeviceEdgePoints), f64p, vp, vp, P(D.TransformStats)]),
    "eg3d_transform_points": (i32, [vp, f64p, f32p, u64, f32p, P(D.TransformStats)]),
}

# include/eg3d_host_transform.h (libeg3d_host.so): the similarity fit to known camera centres, its sequential application
# to points and cameras, the position error, and the same on a loaded SfM object
EG3D_HOST_TRANSFORM = {
    "eg3d_host_read_camera_poses": (i32, [cstr, i32, f64p]),
    "eg3d_host_null_cameras": (i32, [i32, f32p, f32p, u8p]),
    "eg3d_host_similarity_fit": (i32, [i32, f64p, f64p, u8p, f64p, P(D.SimilarityStats)]),
    "eg3d_host_transform_points": (i32, [f64p, f32p, u64, f32p]),
    "eg3d_host_transform_cameras": (i32, [f64p, i32, f32p, f32p, f32p, f32p, f32p]),
    "eg3d_host_glm_inverse4": (i32, [f32p, f32p]),
    "eg3d_host_glm_mul4": (i32, [f32p, f32p, f32p]),
    "eg3d_host_camera_errors": (i32, [i32, f32p, u8p, f64p, f32p]),
    "eg3d_sfm_camera_centres": (i32, [vp, f64p, u8p]),
    "eg3d_sfm_apply_transform": (i32, [vp, f64p, i32]),
}

# header -> (library, table), in the order the headers were added; "eg3d" is both product libraries
HEADERS = {
    "eg3d.h": ("eg3d", EG3D),
    "eg3d_host.h": ("host", EG3D_HOST),
    "eg3d_rccl.h": ("rccl", EG3D_RCCL),
    "eg3d_accumulate.h": ("eg3d", EG3D_ACCUMULATE),
    "eg3d_host_accumulate.h": ("host", EG3D_HOST_ACCUMULATE),
    "eg3d_dedup_phases.h": ("eg3d", EG3D_DEDUP_PHASES),
    "eg3d_host_dedup_phases.h": ("host", EG3D_HOST_DEDUP_PHASES),
    "eg3d_rccl_claims.h": ("rccl", EG3D_RCCL_CLAIMS),
    "eg3d_replay_merge.h": ("eg3d", EG3D_REPLAY_MERGE),
    "eg3d_host_replay_merge.h": ("host", EG3D_HOST_REPLAY_MERGE),
    "eg3d_sets_device.h": ("eg3d", EG3D_SETS_DEVICE),
    "eg3d_triangulate.h": ("eg3d", EG3D_TRIANGULATE),
    "eg3d_host_triangulate.h": ("host", EG3D_HOST_TRIANGULATE),
    "eg3d_colour.h": ("eg3d", EG3D_COLOUR),
    "eg3d_host_colour.h": ("host", EG3D_HOST_COLOUR),
    "eg3d_transform.h": ("eg3d", EG3D_TRANSFORM),
    "eg3d_host_transform.h": ("host", EG3D_HOST_TRANSFORM),
}
FROZEN_HEADERS = ("eg3d.h", "eg3d_host.h", "eg3d_rccl.h")

# include/eg3d/edges.h (libeg3d.so, libeg3d_dlt4x4.so): the 3-D edge model of a graph3d traced and simplified on the device, K17
EDGES = {
    "eg3d_edge_chains_device": (i32, [vp, P(D.DeviceGraph3D), f32, i32, P(D.DeviceEdgeChains), P(D.EdgeChains), P(D.EdgesStats)]),
    "eg3d_edge_chains": (i32, [vp, P(D.Graph3D), f32, i32, P(D.DeviceEdgeChains), P(D.EdgeChains), P(D.EdgesStats)]),
    "eg3d_free_edge_chains": (None, [P(D.EdgeChains)]),
}

# include/eg3d/host_edges.h (libeg3d_host.so): its sequential statement and the PLY line model
HOST_EDGES = {
    "eg3d_host_edge_chains": (i32, [P(D.Graph3D), f32, i32, P(D.EdgeChains), P(D.EdgesStats)]),
    "eg3d_host_free_edge_chains": (None, [P(D.EdgeChains)]),
    "eg3d_host_write_ply_edges": (i32, [cstr, P(D.EdgeChains), f32p]),
}

# The headers that live in subdirectories of include/, as HEADERS: header -> (library, table). bind_library declares these
# as well; tests/test_abi_edges.py holds them to their headers, mirrors (_cdefs.MIRRORS_EXT) and exports.
EXT_HEADERS = {
    "eg3d/edges.h": ("eg3d", EDGES),
    "eg3d/host_edges.h": ("host", HOST_EDGES),
}


# include/eg3d/nearest.hpp (libeg3d.so, libeg3d_dlt4x4.so): a uniform-grid index over a point set and the nearest distances
# of a second point set against it, K18; the index handle (eg3d_cloud_index*) is a void pointer here
NEAREST = {
    "eg3d_cloud_index_build": (i32, [vp, f32p, u64, u8p, f32, P(vp), P(D.CloudIndexStats)]),
    "eg3d_cloud_index_build_device": (i32, [vp, P(D.DeviceEdgePoints), vp, f32, P(vp), P(D.CloudIndexStats)]),
    "eg3d_cloud_index_free": (None, [vp]),
    "eg3d_cloud_nearest_device": (i32, [vp, P(D.DeviceEdgePoints), vp, vp, f32, vp, vp, P(D.NearestStats)]),
    "eg3d_cloud_nearest_points": (i32, [vp, f32p, u64, u8p, vp, f32, f32p, u32p, P(D.NearestStats)]),
}

# include/eg3d/host_nearest.hpp (libeg3d_host.so): its sequential statement and the PLY point reader
HOST_NEAREST = {
    "eg3d_host_nearest_last_error": (cstr, []),
    "eg3d_host_cloud_nearest": (i32, [f32p, u64, u8p, f32p, u64, u8p, f32, f32, f32p, u32p, P(D.NearestStats)]),
    "eg3d_host_cloud_index_stats": (i32, [f32p, u64, u8p, f32, P(D.CloudIndexStats)]),
    "eg3d_host_read_ply_points": (i32, [cstr, P(f32p), u64p]),
    "eg3d_host_free_points": (None, [f32p]),
}

# The .hpp ABI headers (C text under another suffix: the two tests above pin the set of .h files), as HEADERS: header ->
# (library, table). bind_library declares these as well; tests/test_abi_nearest.py holds them to their headers, mirrors
# (_cdefs.MIRRORS_HPP) and exports.
HPP_HEADERS = {
    "eg3d/nearest.hpp": ("eg3d", NEAREST),
    "eg3d/host_nearest.hpp": ("host", HOST_NEAREST),
}


# include/eg3d/edgemap.hh (libeg3d.so, libeg3d_dlt4x4.so): the edge maps of the source images on the device, K19
EDGEMAP = {
    "eg3d_edge_maps": (i32, [i32, C.c_int32, i32p, i32p, P(u8p), P(D.EdgemapParams), P(u8p), P(D.EdgemapStats)]),
}

# include/eg3d/host_edgemap.hh (libeg3d_host.so): their sequential statement, the PNG writer of a mask, the graphs of many masks
HOST_EDGEMAP = {
    "eg3d_host_edgemap_last_error": (cstr, []),
    "eg3d_host_edge_maps": (i32, [C.c_int32, i32p, i32p, P(u8p), P(D.EdgemapParams), P(u8p), P(D.EdgemapStats)]),
    "eg3d_host_png_write_mask": (i32, [cstr, u8p, C.c_int32, C.c_int32]),
    "eg3d_host_plg_build_views_from_masks": (i32, [P(u8p), C.c_int32, i32p, i32p, P(D.PlgView)]),
}

# The open registry, as HEADERS: header -> (library, table). The three registries above are each pinned to a size and a
# suffix by the test that came with them; this one is pinned to neither. The next ABI header — under include/eg3d/, with a
# suffix those tests do not collect — is a new row here and its structs a row of _cdefs.MIRRORS_OPEN; tests/test_abi_open.py
# derives every check from the two.
OPEN_HEADERS = {
    "eg3d/edgemap.hh": ("eg3d", EDGEMAP),
    "eg3d/host_edgemap.hh": ("host", HOST_EDGEMAP),
}


def bind(lib, table):
    """Declare every function of `table` on the CDLL `lib`; a library that lacks one is refused. Returns `lib`."""
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def bind_library(lib, library):
    """Declare on the CDLL `lib` every table HEADERS, EXT_HEADERS, HPP_HEADERS and OPEN_HEADERS give to `library` ("eg3d",
    "host" or "rccl"). Returns `lib`."""
    for owner, table in [row for reg in (HEADERS, EXT_HEADERS, HPP_HEADERS, OPEN_HEADERS) for row in reg.values()]:
        if owner == library:
            bind(lib, table)
    return lib
