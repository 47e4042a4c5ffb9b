/*
 * eg3d.h — C ABI of the MI355X-native EdgeGraph3D hot path
 * (refpoint -> epipolar polyline match -> multi-view edge-point triangulation,
 *  plus the batched Gauss-Newton outlier filter).
 *
 * The reference (abignoli/EdgeGraph3D) has no FFI layer: its seams are C++ free
 * functions and virtual classes. Each entry point below names the reference seam
 * it replaces (paths relative to the reference tree):
 *
 *   eg3d_create / eg3d_clone / eg3d_destroy
 *       context construction in edge_matching(): PolyLine2DMapSearch per view at
 *       4 px (src/edgegraph3d/edge_matcher.cpp:101-103), PLGEdgeManager ctor with
 *       the 30 px maps (edge_managers/plg_edge_manager.cpp:46-75),
 *       PLGPCM3ViewsPLGFollowing ctor (edge_matcher.cpp:115).
 *   eg3d_candidates
 *       PLGEdgeManager::detect_nearby_intersections_and_correspondences_plgp(int)
 *       (include/.../plg_edge_manager.hpp:74, plg_edge_manager.cpp:261-300).
 *   eg3d_match_refpoints
 *       plg_matching_from_refpoints[_parallel](sfmd, em, cm, plgmm)
 *       (include/.../plg_matching_from_refpoints.hpp:53,55;
 *        src/.../plg_matching_from_refpoints.cpp:64-116).
 *   eg3d_gn_filter
 *       gaussNewtonFiltering(SfMData&, vector<bool>&, float)
 *       (include/edgegraph3d/filtering/gauss_newton.hpp:20; gauss_newton.cpp:136-178).
 *   eg3d_get_grid
 *       read-back of PolyLine2DMap::pls_id_maps (matching/plg_matching/polyLine_2d_map.cpp:40-58)
 *       so the grid membership can be checked against the CPU oracle.
 *
 * Conventions: plain C, POD structs, caller-owned input buffers that must stay
 * valid for the duration of the call only (eg3d_create copies the scene to HBM).
 * Status: 0 = ok, <0 = error (eg3d_last_error() gives text). One context per GPU;
 * a context is thread-compatible (one caller thread at a time), like the reference.
 * Ids that are `ulong` in the reference are uint32_t here (documented narrowing).
 */
#ifndef EG3D_H_
#define EG3D_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EG3D_OK 0
#define EG3D_ERR_ARG -1
#define EG3D_ERR_HIP -2
#define EG3D_ERR_CAPACITY -3 /* a device-side fixed capacity was exceeded; flags say which */
#define EG3D_ERR_NODEVICE -4
#define EG3D_ERR_HOSTONLY -5 /* the input needs the host form of the entry point (eg3d_replay_device) */

/* ---------------------------------------------------------------- scene ---- */
/* Flat, read-only description of everything the path reads besides the seeds.
 * Replaces SfMData::camerasList_[v].cameraMatrix, `Mat** F` and
 * vector<PolyLineGraph2DHMapImpl> (reference: SfMData.h:16-30,
 * types_reconstructor.hpp:68-82, polyline_graph_2d.hpp:85-119,278-294). */
typedef struct eg3d_scene {
  int32_t n_views;            /* <= 8192; a view holds <= 524 288 polylines (EG3D_ERR_CAPACITY otherwise) */
  int32_t width, height;      /* image size, identical for all views (imgs[0].size()) */
  const float* cam_P;         /* [V][16] cameraMatrix[r][c], row-major 4x4, last row 0 (Q6) */
  const double* F;            /* [V][V][9] row-major; F[i][j] maps a point of view i to its line in view j */
  const uint8_t* F_valid;     /* [V][V] 0 => "1x1 Mat" => epiline fails (geometric_utilities.cpp:826,840) */
  const uint32_t* view_pl_off;/* [V+1] polyline index range of each view in the arrays below */
  const uint32_t* pl_vtx_off; /* [NP+1] vertex range of each polyline (global indices into vtx_xy) */
  const float* vtx_xy;        /* [NV][2] polyline_coords; on valid polylines finite and within +-1e7 px (eg3d_create refuses
                                 the scene otherwise: the reference's grid sampling does not terminate on such input) */
  const uint32_t* pl_start;   /* [NP] node id `start` */
  const uint32_t* pl_end;     /* [NP] node id `end`   */
  const uint8_t* pl_valid;    /* [NP] PolyLineGraph2D::is_valid_polyline (polyline_graph_2d.cpp:1141-1147); the vertices of an
                                 invalid polyline, if the caller left any, are ignored (an invalidated polyline of the
                                 reference has none) */
} eg3d_scene;

/* Seeds = SfM reference points: camViewingPointN_ + point2DoncamViewingPoint_ as CSR. */
typedef struct eg3d_seeds {
  uint32_t n_seeds;
  const uint32_t* trk_off;    /* [N+1] */
  const int32_t* trk_view;    /* [trk_off[N]] view ids, in the order stored in the SfM file */
  const float* trk_xy;        /* [trk_off[N]][2] */
} eg3d_seeds;

/* ------------------------------------------------------------- outputs ----- */
/* Edge-points = vector<tuple<vec3, vector<plg_point>, vector<int>>> of the reference,
 * flattened. Library-owned; release with eg3d_free_edgepoints. Order is the
 * reference's emission order (seed, start view in track order, start hit in
 * ascending polyline id, chain order). */
typedef struct eg3d_edgepoints {
  uint64_t n_points;
  uint64_t n_obs;
  float* X;            /* [n_points][3] */
  uint64_t* obs_off;   /* [n_points+1]; 64-bit: the cloud of one call may hold more than 2^32 observations
                          (BASELINE config 4 as one call: 56 M points, 4.1 G observations) */
  int32_t* obs_view;   /* [n_obs] */
  uint32_t* obs_pl;    /* [n_obs] polyline id inside its view */
  uint32_t* obs_seg;   /* [n_obs] segment index */
  float* obs_xy;       /* [n_obs][2] */
  uint32_t* key;       /* [n_points][4] seed, start-view index in track, start-hit index, index in chain */
  uint64_t n_tasks;        /* (seed, start view, start hit) tasks examined */
  uint64_t n_hypotheses;   /* 3-view hypotheses evaluated */
  uint64_t n_chains;       /* chains emitted */
  uint32_t flags;          /* EG3D_FLAG_* capacity / quirk indicators */
  void* _owner;            /* internal */
} eg3d_edgepoints;

#define EG3D_FLAG_CHAIN_OVERFLOW   1u  /* a chain exceeded the device chain capacity */
#define EG3D_FLAG_OBS_OVERFLOW     2u  /* a chain's observation pool was exhausted   */
#define EG3D_FLAG_HYP_OVERFLOW     4u  /* a following direction exceeded its capacity */
#define EG3D_FLAG_DIR_MISMATCH     8u  /* Q15: a walk was asked to follow a node id that is neither end of its polyline */
#define EG3D_FLAG_DEGENERATE_DLT  16u  /* Q11: a DLT initialisation used the same camera twice */

/* Stage A result for one seed range (testable alone). Library-owned. */
typedef struct eg3d_candidates {
  uint32_t n_sv;            /* number of (seed, track entry) pairs = trk_off[end]-trk_off[begin] */
  uint32_t* cand_off;       /* [n_sv+1] candidate polylines (<= 30 px), ascending id */
  uint32_t* cand_pl;
  uint32_t* start_off;      /* [n_sv+1] starting intersections (<= 10 px) */
  uint32_t* start_pl;
  uint32_t* start_seg;
  float* start_xy;          /* [..][2] */
  /* per starting intersection (task), per track entry of the seed: epipolar hits */
  uint32_t n_tasks;
  uint32_t* task_sv;        /* [n_tasks] index of the (seed,view) pair the task starts from */
  uint32_t* task_hit;       /* [n_tasks] index of the start hit inside that pair */
  uint32_t* task_list_off;  /* [n_tasks+1] offset into list_off: one list per track entry */
  uint32_t* list_off;       /* [n_lists+1] */
  uint32_t* hit_pl;
  uint32_t* hit_seg;
  float* hit_xy;
  void* _owner;
} eg3d_candidates;

typedef struct eg3d_ctx eg3d_ctx;

/* Per-call timing of the device stages, filled by eg3d_match_refpoints (ms, HIP events
 * on the context's stream). */
typedef struct eg3d_stage_times {
  float ms_total;
  float ms_candidates;   /* K1 seed_candidates (count+fill) */
  float ms_epipolar;     /* K2 epipolar_hits (count+fill)   */
  float ms_hypotheses;   /* K3a consensus hypotheses        */
  float ms_select;       /* K3s uniqueness / chain assembly */
  float ms_expand;       /* K3b expand-all-views            */
  float ms_emit;         /* K4 compaction                   */
  uint64_t bytes_algorithmic; /* SURVEY 8(d) algorithmic bytes of this call */
  float ms_slowest_chain; /* the longest time ONE chain held its wavefront in the expand stage: a lower bound of every
                             expand launch, whatever else the GPU is doing (appended in round 6: the struct grew, rebuild callers) */
} eg3d_stage_times;

const char* eg3d_last_error(void);
int eg3d_device_count(void);
/* Form of the 2-view DLT that initialises every triangulation (cv::triangulatePoints,
 * triangulation.cpp:216,290), fixed when the library is built: 2 = rows x*P2-P0, y*P2-P1 per view
 * (4x4 system, later OpenCV releases), 3 = those plus x*P1-y*P0 (6x4, OpenCV 2.4-3.1, the release
 * the reference names). The reference pins no OpenCV version; see DESIGN.md 3. */
int eg3d_dlt_rows(void);

int eg3d_create(const eg3d_scene* scene, int device, eg3d_ctx** out);
void eg3d_destroy(eg3d_ctx* ctx);

/* A second context on the same device that SHARES `parent`'s immutable scene and its currently
 * resident seeds (reference-counted; either may be destroyed first) but has its own HIP stream,
 * events and work buffers. Seeds are independent units on this path
 * (plg_matching_from_refpoints.cpp:83-104 loops over them with no carried state), so a host keeps
 * several batches in flight by driving one context per thread; eg3d_upload_seeds on one context
 * does not affect the others. */
int eg3d_clone(eg3d_ctx* parent, eg3d_ctx** out);

/* which: 0 = 30 px candidate grid, 1 = 4 px expand-all-views grid, 2 = 10 px map of eg3d_match_polylines_closeness (exists
 * after the first such call; EG3D_ERR_ARG before). Pointers stay
 * valid until eg3d_destroy. cell index = row*ncols + col. (The grids are built and kept on the device; the first call for a
 * cell size copies that grid to the host.) */
int eg3d_get_grid(eg3d_ctx* ctx, int view, int which, uint32_t* ncols, uint32_t* nrows,
                  const uint32_t** cell_off, const uint32_t** ids);

int eg3d_candidates_run(eg3d_ctx* ctx, const eg3d_seeds* seeds, uint32_t seed_begin,
                        uint32_t seed_end, eg3d_candidates* out);
void eg3d_free_candidates(eg3d_candidates* c);

/* Full path on seeds [seed_begin, seed_end). With device_only != 0 the result stays
 * in HBM (out->X etc. are NULL, counts are filled) — used for kernel-only timing. */
int eg3d_match_refpoints(eg3d_ctx* ctx, const eg3d_seeds* seeds, uint32_t seed_begin,
                         uint32_t seed_end, int device_only, eg3d_edgepoints* out,
                         eg3d_stage_times* times /* may be NULL */);
/* Pipelines 1-2 extractor:
 * find_new_3d_points_from_compatible_polylines_expandallviews_parallel
 * (src/edgegraph3d/matching/plg_matching/polyline_matching.cpp:153-208, called per set from
 * pipelines.cpp:98,144) with find_epipolar_correspondences (:45-73). A set of "potentially
 * compatible polylines" is, per view, an ascending list of view-local polyline ids (the
 * reference's vector<set<ulong>>). Every polyline of a set is sampled every 20 px from its start
 * to its end; each sample collects the hits of its epipolar line on the set's polylines of all
 * other views and goes through the same 3-view consensus + expand-all-views as a seed's starting
 * hit. This call does not consult a PLGMatchesManager (is_matched() == false: the manager is empty when the
 * reference's edge_matching() runs pipelines 1-2 and is never updated inside the loop);
 * eg3d_match_polyline_sets_matched below does, for a caller that holds a filled one.
 * Output as eg3d_match_refpoints, in the reference's order (set, start view, polyline id, sample);
 * key = (sample index of the call, start view, 0, index in chain), in the host arrays and in the
 * device view (eg3d_last_device_output after device_only) alike. */
typedef struct eg3d_polyline_sets {
  uint32_t n_sets;
  const uint32_t* row_off; /* [n_sets * n_views + 1] CSR over rows (set * n_views + view) */
  const uint32_t* pl_ids;  /* view-local polyline ids, strictly ascending within a row (a set: no repeats;
                              EG3D_ERR_ARG otherwise) */
} eg3d_polyline_sets;
int eg3d_match_polyline_sets(eg3d_ctx* ctx, const eg3d_polyline_sets* sets, uint32_t set_begin, uint32_t set_end,
                             int device_only, eg3d_edgepoints* out, eg3d_stage_times* times);
/* The same extractor for a caller whose PLGMatchesManager already holds matched intervals (pipeline 3 ran first, a re-run on
 * new polyline matches, chains added between sets): plgmm.is_matched is asked where the reference asks it
 * (polyline_matching.cpp:175 and :65; the rule with its quirks M1-M4: csrc/eg3d_matched_core.h).
 *   - a 20 px sample inside a held interval never becomes a task; the walk goes on from
 *     next_pl_point_by_distance(interval.end, pl.end, 20) (:186-189);
 *   - an epipolar hit inside a held interval is dropped from its list.
 * key[0] counts the samples that became tasks; order and everything else as eg3d_match_polyline_sets. `m` is the
 * matched_polyline_intervals CSR of a host graph, struct eg3d_graph3d: host arrays, uploaded for the duration of the call; or of the
 * eg3d_device_graph3d of eg3d_replay_device on ctx's device (read in place). m == NULL or a table without intervals: exactly
 * eg3d_match_polyline_sets. The table is checked before anything is indexed with it (EG3D_ERR_ARG, `out` untouched):
 * struct_size, n_scene_polylines, offsets ascending, both segment indices of every interval inside its polyline, start
 * segments strictly ascending within a row. A walk that would not advance (an interval whose end lies behind the point it
 * contains — the reference does not terminate on it) is refused as EG3D_ERR_ARG too: the intervals do not belong to
 * this scene. */
typedef struct eg3d_matched_intervals {
  uint32_t struct_size;        /* sizeof(eg3d_matched_intervals) */
  int32_t on_device;           /* pointers are HBM of ctx's device (an eg3d_device_graph3d), else host */
  uint64_t n_scene_polylines;  /* must equal view_pl_off[V] */
  const uint64_t* iv_off;      /* [n_scene_polylines + 1] */
  const uint32_t* iv_start_seg;
  const float* iv_start_xy;    /* [..][2] */
  const uint32_t* iv_end_seg;
  const float* iv_end_xy;
} eg3d_matched_intervals;
int eg3d_match_polyline_sets_matched(eg3d_ctx* ctx, const eg3d_polyline_sets* sets, uint32_t set_begin, uint32_t set_end,
                                     const eg3d_matched_intervals* m /* NULL = none */, int device_only,
                                     eg3d_edgepoints* out, eg3d_stage_times* times);
/* Stage A of the extractor alone (as eg3d_candidates_run for seeds), in task order. Library-owned. */
typedef struct eg3d_set_candidates {
  uint32_t n_tasks;          /* samples that became tasks */
  int32_t* task_view;        /* [n_tasks] */
  uint32_t* task_pl;         /* [n_tasks] view-local polyline id */
  uint32_t* task_seg;
  float* task_xy;            /* [n_tasks][2] */
  uint64_t* list_off;        /* [n_tasks * n_views + 1] hits of list task * n_views + view */
  uint32_t* hit_pl;
  uint32_t* hit_seg;
  float* hit_xy;             /* [..][2] */
  uint64_t n_samples_skipped;/* samples inside a held interval */
  uint64_t n_hits_filtered;  /* epipolar hits inside a held interval */
  void* _owner;
} eg3d_set_candidates;
int eg3d_polyline_set_candidates(eg3d_ctx* ctx, const eg3d_polyline_sets* sets, uint32_t set_begin, uint32_t set_end,
                                 const eg3d_matched_intervals* m /* NULL = none */, eg3d_set_candidates* out);
void eg3d_free_set_candidates(eg3d_set_candidates* c);
/* The checks of `sets` that need no device and no scene (eg3d_match_polyline_sets runs them too, after its id-range
 * check): row_off ascending, ids strictly ascending within every row. EG3D_OK or EG3D_ERR_ARG (eg3d_last_error says
 * which). Usable without a GPU. */
int eg3d_check_polyline_sets(const eg3d_polyline_sets* sets, int32_t n_views);

void eg3d_free_edgepoints(eg3d_edgepoints* e);

/* Resident-seed variant: upload once, run many times (bench: inputs in HBM before the
 * timed region). */
int eg3d_upload_seeds(eg3d_ctx* ctx, const eg3d_seeds* seeds);
int eg3d_match_resident(eg3d_ctx* ctx, uint32_t seed_begin, uint32_t seed_end, int device_only,
                        eg3d_edgepoints* out, eg3d_stage_times* times);

/* Internal pipelining of ONE eg3d_match_* call. The reference's parallel entry point runs the seeds of a call on its OpenMP
 * team (plg_matching_from_refpoints.cpp:83-104, `#pragma omp parallel for`; polyline_matching.cpp:153-208 for the sets);
 * here a call's range is cut into `units` contiguous sub-batches (balanced by the sum of track lengths / polylines) that
 * run concurrently on `lanes` internal contexts (own HIP stream, work buffers and host thread, created on first use,
 * shared scene and seeds), so that the candidate / hypothesis stages and the D2H copy of one sub-batch overlap the expand
 * stage of another. The output is the concatenation of the sub-batches in order: byte for byte what a single batch
 * produces. lanes: 1 = no pipelining (the call runs on the context's own stream, one batch of <= 16 384 seeds at a time),
 * 0 = the default, by the kind of call (EG3D_PIPELINE_LANES overrides): 3 for a call that copies its cloud to the host —
 * most of the D2H copy disappears behind the later sub-batches — on a context that has ALREADY completed a host call (lanes
 * cost 50-90 ms, on many-view scenes seconds, when they are created: a one-shot caller's only call runs on the context
 * alone), and 1 for a device-only call, which measured no gain (every expand launch lasts at least as long as its slowest
 * chain: eg3d_stage_times.ms_slowest_chain); units: 0 = chosen
 * from the range (one per lane when each gets >= 128 seeds; EG3D_PIPELINE_UNITS). A clone inherits its parent's setting. Use lanes = 1 on contexts that are themselves driven
 * concurrently (one per host thread): stacking both forms of overlap only multiplies the work buffers. */
int eg3d_set_pipelining(eg3d_ctx* ctx, int lanes, int units);

/* Device-resident view of the edge-points produced by the most recent eg3d_match_* call
 * (pointers into the context's HBM buffers, valid until the next call on this context).
 * A call made with device_only != 0 keeps its WHOLE result in these buffers however many internal
 * sub-batches (<= 16 384 seeds, one expand launch each) it took (global 64-bit observation offsets;
 * obs_off has n_points entries, no sentinel) and `complete` is 1 — this is what the multi-GPU exchange
 * of the edge-point cloud consumes without a host trip; the buffers grow to the size of the call's
 * cloud (12 + 8 + 16 B per point, 20 B per observation). A call that copies to the host
 * (device_only == 0) reuses the buffers per sub-batch: `complete` is then 1 only if it ran as a single one. */
typedef struct eg3d_device_edgepoints {
  uint64_t n_points, n_obs;
  const float* X;
  const uint64_t* obs_off;
  const int32_t* obs_view;
  const uint32_t* obs_pl;
  const uint32_t* obs_seg;
  const float* obs_xy;
  const uint32_t* key;
  int32_t complete;
} eg3d_device_edgepoints;
int eg3d_last_device_output(eg3d_ctx* ctx, eg3d_device_edgepoints* out);

/* Config 5: batched FP32 Gauss-Newton filter. view ids index ctx's cameras.
 * X_out may alias X. legacy_abs != 0 selects the Q9 integer-abs behaviour. */
int eg3d_gn_filter(eg3d_ctx* ctx, const float* X, const uint32_t* obs_off, const int32_t* obs_view,
                   const float* obs_xy, uint64_t n_points, float gn_max_mse, int legacy_abs,
                   float* X_out, uint8_t* inlier, float* ms_kernel /* may be NULL */);

/* The view count of the context's scene and the HIP device it lives on (either pointer may be NULL); clones answer too. */
int eg3d_context_info(eg3d_ctx* ctx, int32_t* n_views, int32_t* device);

/* ---- the filter stage on a device-resident cloud ------------------------------------------------------------------
 * gaussNewtonFiltering, the observation-count filter and the copy of the survivors (gauss_newton.cpp:136-178,
 * outliers_filtering.cpp:14-114) on a cloud that is already in HBM: this context's last output after a device_only call,
 * the result of the multi-GPU gather or concatenation (include/eg3d_rccl.h), or caller-built device arrays. Offsets are
 * 64-bit without a sentinel (the last point ends at n_obs), so clouds of 2^32 observations and more pass. Nothing is
 * validated on the host: the kernels check what they index, and a view id outside the context's rig, offsets that do not
 * ascend within [0, n_obs] or a single list of more than 2^24 observations fail the call with EG3D_ERR_ARG (the outputs
 * are then unspecified). One caller thread at a time per context, as everywhere. Caller-built arrays must be aligned as
 * hipMalloc aligns them, at least to their element: 4 bytes for X, key, obs_view, obs_pl and obs_seg, 8 bytes for obs_off and
 * for obs_xy (an (x, y) pair moves as one 8-byte word).
 *
 * Order of the reference: it removes points whose observations fall within 3 px of an earlier point's
 * (filter_3d_points_close_2d_array) BEFORE it filters. The Gauss-Newton verdict of a point depends on that point alone, so
 * the reference-exact sequence, all of it on the device, is
 *   1. eg3d_dedup_device -> its mask as keep_dev -> the Gauss-Newton filter below;
 *   2. the compaction with keep = dedup AND inlier (what the masked filter writes), min_obs = the observation threshold;
 * eg3d_dedup_resident (at the end of this header) runs exactly this on the context's last device output. The host
 * library's filter_close_2d step gives the same mask from a host copy of the cloud.
 *
 * Gauss-Newton filter. keep_dev: optional device byte mask, NULL = all points; a masked-out point costs no arithmetic, gets
 * inlier 0 and X_out = X. Per point the arithmetic is that of the host-array entry point above, bit for bit (both abs
 * behaviours of Q9). X_out_dev ([n_points][3]) may alias cloud->X; inlier_dev is [n_points]. obs_hist_host, optional,
 * [n_views + 1]: entry k = number of inliers with k observations; lists longer than n_views go to no bin, as in the host
 * library's observation filter. n_inliers_host, optional: the number of ALL inliers, those of no bin included — the count
 * the threshold rule needs beside the histogram, without a copy of inlier_dev. */
int eg3d_gn_filter_device(eg3d_ctx* ctx, const eg3d_device_edgepoints* cloud, const uint8_t* keep_dev, float gn_max_mse,
                          int legacy_abs, float* X_out_dev, uint8_t* inlier_dev, uint64_t* obs_hist_host /* may be NULL */,
                          uint64_t* n_inliers_host /* may be NULL */, float* ms_kernel /* may be NULL */);
/* Order-preserving stream compaction of all seven arrays: keeps the points with keep_dev[i] != 0 (NULL = all) AND more than
 * min_obs observations (min_obs < 0: no count test); X_new_dev, if given, replaces X. The result lives in buffers of the
 * context that are separate from the match output, and is valid until the next compaction on this context or its
 * destruction; complete = 1 and obs_off has no sentinel, so it feeds the multi-GPU gather unchanged. `out` must not alias
 * `cloud`, and `cloud` must not view the result of an earlier compaction on this context (EG3D_ERR_ARG). */
int eg3d_compact_device(eg3d_ctx* ctx, const eg3d_device_edgepoints* cloud, const uint8_t* keep_dev,
                        const float* X_new_dev /* may be NULL */, int32_t min_obs, eg3d_device_edgepoints* out);
/* Filled by the composition below. struct_size: the CALLER sets it to sizeof(eg3d_filter_stats) before the call; a value
 * smaller than the library's struct is refused with EG3D_ERR_ARG before anything is written (new members are appended). */
typedef struct eg3d_filter_stats {
  uint32_t struct_size;
  int32_t threshold;       /* a point is kept with MORE observations than this */
  uint64_t n_points_in;    /* points of the cloud */
  uint64_t n_masked_in;    /* ... that the keep mask let through (no mask here: all) */
  uint64_t n_gn_inliers;   /* ... accepted by the Gauss-Newton filter */
  uint64_t n_kept;         /* ... that also passed the observation threshold */
  uint64_t n_obs_kept;     /* observations of the kept points */
  float ms_filter;         /* the filter kernel (HIP events) */
  float ms_compact;        /* the three compaction launches and the read-back of their totals (HIP events) */
  float ms_copy;           /* the copy of the survivors to the host (wall; 0 without to_host) */
} eg3d_filter_stats;
/* Convenience composition on the context's last device output (which must be `complete`): Gauss-Newton filter WITHOUT a
 * mask, threshold by the rule of the host library's observation filter over the histogram of the inliers plus base_hist
 * (optional, [n_views + 1], entry k = the caller's SfM points with k observations, which the reference counts in the same
 * histogram): the median bin, max(3, median / 2 - 1), overridden by forced_min_filter > -1; compaction; with to_host a copy
 * of the survivors into a library-owned cloud (obs_off with its sentinel; release with eg3d_free_edgepoints). out_host is
 * required with to_host; out_dev and stats may be NULL. This filters the cloud as matched, NOT deduplicated: the reference's
 * filter step, which dedups first, is eg3d_dedup_resident below (see the order above). */
int eg3d_filter_resident(eg3d_ctx* ctx, float gn_max_mse, int legacy_abs, int forced_min_filter, const uint64_t* base_hist,
                         int to_host, eg3d_edgepoints* out_host, eg3d_device_edgepoints* out_dev, eg3d_filter_stats* stats);

/* ---- the 3 px de-duplication on a device-resident cloud ------------------------------------------------------------
 * filter_3d_points_close_2d_array (filtering_close_plgps.cpp:75-124): every view carries an occupancy grid of 3 px cells,
 * w = ceil((float)width / 3) by h = ceil((float)height / 3); in cloud order a point is kept when one of its observations
 * falls into a cell no earlier kept point occupies, and a kept point occupies the cells of all its observations. The first
 * point that touches a cell is always kept, so the rule is order-independent: keep[i] = some observation of i lies in a
 * cell whose smallest touching point index is i. The context owns a claim map of those minima (one uint32 per cell of
 * every view, created on first use: 4 * n_views * w * h bytes; a clone has its own, empty at first).
 *
 * Writes the byte mask keep_dev[n_points] (device memory) and, if given, the number of kept points to *n_kept_host.
 * reset != 0 clears the claim map first; otherwise the claims of the earlier calls on this context stand, and the points
 * of this cloud are numbered from index_base. Contract: the dedup of cloud A (reset, index_base 0) and then of cloud B
 * (no reset, index_base = |A|) gives the two halves of the mask of the concatenation A || B - the reference dedups the
 * concatenation of its three pipeline stages this way (pipelines.cpp:219-239). index_base + n_points must stay below
 * 2^32 - 1: EG3D_ERR_ARG otherwise, before anything is launched. An observation with a view id outside the rig, or with
 * coordinates outside the grid (x / 3 or y / 3 not inside (-1, w) x (-1, h), NaN included), is NOT an error here, unlike in
 * the filter: it claims nothing and keeps nothing, the rule of the host step and of the CPU oracle; a point with an empty
 * list is dropped. Offsets that do not ascend within [0, n_obs] fail the call with EG3D_ERR_ARG (device-side check). A
 * call that fails after its arguments were accepted, for this or any other reason, discards its claims with all earlier
 * ones: the next call on the context starts from an empty map whatever its `reset`. cloud->obs_pl,
 * obs_seg and key are not read. */
int eg3d_dedup_device(eg3d_ctx* ctx, const eg3d_device_edgepoints* cloud, uint64_t index_base, int reset,
                      uint8_t* keep_dev, uint64_t* n_kept_host /* may be NULL */);
/* Filled by eg3d_dedup_resident. struct_size as in eg3d_filter_stats: set by the caller, a smaller value is refused. */
typedef struct eg3d_dedup_stats {
  uint32_t struct_size;
  int32_t threshold;       /* the observation threshold (kept: MORE observations than this); -1 without the filter */
  uint64_t n_points_in;    /* points of the cloud */
  uint64_t n_dedup_kept;   /* ... kept by the dedup */
  uint64_t n_gn_inliers;   /* ... of those accepted by the Gauss-Newton filter (0 without the filter) */
  uint64_t n_kept;         /* points of the result */
  uint64_t n_obs_kept;     /* observations of the result */
  float ms_dedup;          /* the two dedup kernels (HIP events; the fill of a reset map precedes them) */
  float ms_filter;         /* the filter kernel (HIP events; 0 without the filter) */
  float ms_compact;        /* the compaction, as in eg3d_filter_stats */
  float ms_copy;           /* the copy of the survivors to the host (wall; 0 without to_host) */
} eg3d_dedup_stats;
/* The reference's dedup + filter on the context's last device output (which must be `complete`), without the host in it:
 * eg3d_dedup_device with the caller's reset and index_base; with with_filter != 0 the Gauss-Newton filter with the dedup
 * mask as keep_dev and the observation threshold by the rule of eg3d_filter_resident (base_hist, forced_min_filter as
 * there); eg3d_compact_device with the resulting mask (and the filter's new X); with to_host a copy of the survivors
 * into a library-owned cloud (release with eg3d_free_edgepoints). out_host is required with to_host; out_dev and stats may
 * be NULL. The result lives in the compaction's buffers: valid until the next compaction on this context. If a step after
 * the dedup fails (the filter refuses a view id outside the rig, which the dedup tolerates), the claims are discarded as
 * after a failed eg3d_dedup_device. */
int eg3d_dedup_resident(eg3d_ctx* ctx, uint64_t index_base, int reset, int with_filter, float gn_max_mse, int legacy_abs,
                        int forced_min_filter, const uint64_t* base_hist, int to_host, eg3d_edgepoints* out_host,
                        eg3d_device_edgepoints* out_dev, eg3d_dedup_stats* stats);

/* ---- the PLGMatchesManager replay (row a17) on a device-resident cloud ---------------------------------------------
 * What plgmm.add_matched_3dpolyline leaves behind when the reference runs the path (plg_matches_manager.cpp:99-180): the
 * 3-D polyline graph the reference serialises as outgraph.3dg, and the matched 2-D intervals per (view, polyline). The
 * result is the eg3d_graph3d of include/eg3d_host.h, field for field and byte for byte what the host library's
 * eg3d_host_replay_matches builds from a host copy of the same cloud; it needs the WHOLE cloud as matched, not the
 * survivors of the dedup or the filter, and on the device only the graph has to travel. `cloud`: NULL = this context's last
 * device output (which must be `complete`), or the result of eg3d_compact_device, of the multi-GPU gather or concatenation
 * (include/eg3d_rccl.h), or caller-built device arrays under the alignment contract of the filter stage; offsets are 64-bit
 * without a sentinel. This call builds the graph of ONE cloud; a graph that accumulates over the calls of a run is
 * eg3d_replay_accumulate (include/eg3d_accumulate.h), which does not disturb this call's state or result.
 *
 * The rules, in the order-independent form the kernels use (host/replay.cpp is the sequential statement): a pair is
 * (i - 1, i) with equal key[0..2] and key[3] counting up by one. Two points are one node when the bit patterns of their
 * (x, y, z) are equal, -0 counting as +0; node ids count the nodes by their first point in cloud order, node_X holds that
 * point's coordinates as stored, node_point the LAST point of the node. A polyline is a distinct unordered pair of nodes
 * (a loop on one node is allowed and linked once), numbered by its first pair and oriented as that pair; conn lists a
 * node's polylines in ascending id. Of the intervals that start on one segment of one scene polyline the first in the
 * order (pair, view ascending) is kept (the reference's std::set compares the start segment only); where a point lists a
 * view twice, the last observation counts.
 *
 * Refused, by device-side checks that run before anything is indexed or written (out_dev, out_host and stats are left
 * untouched and the result of an earlier replay stays valid):
 *   EG3D_ERR_HOSTONLY  a NaN coordinate, or an x or y equal to -1.0f (the reference's INVALID_POINT_COORDS), in the X of a
 *                      point that belongs to a pair: the reference then makes a new node on every lookup and wipes the
 *                      earlier ones, which the rules above do not cover. Copy such a cloud to the host and give it to
 *                      eg3d_host_replay_matches. The same values in a point of no pair are never looked up and pass.
 *   EG3D_ERR_ARG       a view id outside the rig, a polyline id outside its view, a segment index outside its polyline or
 *                      on a polyline with fewer than two vertices (an invalid polyline of the scene has none here), offsets
 *                      that do not ascend within [0, n_obs]; it takes precedence over EG3D_ERR_HOSTONLY (the host form
 *                      refuses such a cloud too);
 *   EG3D_ERR_CAPACITY  n_points >= 0xfffffff0: node and polyline ids are 32-bit (the host form answers -3).
 * out_dev: the graph in buffers of the context that are separate from the match output and the compaction output, valid
 * until the next replay on this context. out_host: a library-owned copy, released with eg3d_free_graph3d (NOT with the
 * host library's function: libeg3d.so does not depend on libeg3d_host.so). Any of out_dev, out_host, stats may be NULL.
 * EG3D_REPLAY_TABLE_BITS=b (read when the context is created; tests) asks for a node table of 2^b slots; it is raised to
 * the smallest power of two above the number of lookups (two per pair), so small values make the probe sequences long. */
struct eg3d_graph3d;
typedef struct eg3d_device_graph3d { /* the members of eg3d_graph3d, the pointers into HBM */
  uint64_t n_nodes;
  uint64_t n_real_nodes;       /* = n_nodes: no node is ever invalidated on this path (see EG3D_ERR_HOSTONLY) */
  const float* node_X;         /* [n_nodes][3] */
  const uint64_t* node_point;  /* [n_nodes] */
  uint64_t n_polylines;
  const uint32_t* pl_start;    /* [n_polylines] */
  const uint32_t* pl_end;
  const uint64_t* conn_off;    /* [n_nodes + 1] */
  const uint32_t* conn_pl;     /* [conn_off[n_nodes]] */
  uint64_t n_scene_polylines;
  const uint64_t* iv_off;      /* [n_scene_polylines + 1] */
  const uint32_t* iv_start_seg;/* [iv_off[n_scene_polylines]] */
  const float* iv_start_xy;    /* [..][2] */
  const uint32_t* iv_end_seg;
  const float* iv_end_xy;
} eg3d_device_graph3d;
/* struct_size as in eg3d_filter_stats: set by the caller, a smaller value is refused before anything is written. */
typedef struct eg3d_replay_stats {
  uint32_t struct_size;
  uint64_t n_pairs;        /* consecutive chain-point pairs replayed */
  uint64_t n_nodes, n_polylines, n_intervals;
  uint64_t table_slots;    /* node table capacity actually used (0 for a cloud without pairs) */
  float ms_graph;          /* nodes, polylines and connections (HIP events; the small read-backs between the passes included) */
  float ms_intervals;      /* the interval claims, their scan and the records (HIP events) */
  float ms_copy;           /* the copy of the graph to the host (wall; 0 without out_host) */
} eg3d_replay_stats;
int eg3d_replay_device(eg3d_ctx* ctx, const eg3d_device_edgepoints* cloud, eg3d_device_graph3d* out_dev,
                       struct eg3d_graph3d* out_host, eg3d_replay_stats* stats);
void eg3d_free_graph3d(struct eg3d_graph3d* g);

/* ---- pipeline 2: polyline matching by closeness to the reference points ---------------------------------------------
 * polyline_matching_closeness_to_refpoints (src/edgegraph3d/matching/polyline_matching/polyline_matcher.cpp:75-168, called
 * from pipelines.cpp:113-158), on the device. For every seed of [seed_begin, seed_end), ascending, and every entry of its
 * track, the polylines within 10 px of the point's observation in that view are looked up on a 10 px map
 * (PolyLine2DMapSearch with FIND_WITHIN_DIST, polyLine_2d_map_search.cpp:46-77,122-137; the observation of a view is the
 * one eg3d_match_refpoints uses). With n = the track's length, the point is accepted when no entry finds more than one
 * polyline, the distinct (view, polyline) pairs found are at least 0.7 n and at least two, and neither min < max / 3 nor
 * max > 3 min holds for the distances (float, max starting at FLT_MIN: a point whose distances are all 0 is rejected, as in
 * the reference). The pairs of an accepted point are a clique of the match graph; the result lists the graph's connected
 * components in the reference's order (by the first accepted point that names one of their polylines, then by (view,
 * polyline)), each as one ascending id set per view: exactly the rows of an eg3d_polyline_sets, so
 *     eg3d_polyline_sets s = {m.n_sets, m.row_off, m.pl_ids};  eg3d_match_polyline_sets(ctx, &s, 0, s.n_sets, ...);
 * runs the reference's pipeline 2 end to end. The 10 px map is built by the first call on the context or on one of its
 * clones, which then share it (stats->ms_grid: that call only); eg3d_get_grid(which = 2) reads it back from then on and
 * answers EG3D_ERR_ARG before. An empty range, or no accepted point: n_sets = 0, row_off = {0}, EG3D_OK. A track view id
 * outside the rig: EG3D_ERR_ARG, by a device-side check that runs before anything else reads the ids (`out` and `stats`
 * are left untouched; the seeds uploaded before stay in place, as after any refused eg3d_upload_seeds). stats->ms_search is the
 * search kernel alone, ms_components everything between it and the copy. seeds == NULL: the seeds uploaded last (eg3d_upload_seeds). One caller thread per context. */
typedef struct eg3d_polyline_matches {   /* library-owned; eg3d_free_polyline_matches */
  uint32_t n_refpoints;  uint32_t* refpoints;       /* accepted reference points, ascending */
  uint32_t n_sets;       uint32_t* row_off;         /* [n_sets * n_views + 1] */
  uint32_t* pl_ids;                                 /* as eg3d_polyline_sets */
} eg3d_polyline_matches;
typedef struct eg3d_polymatch_stats { uint32_t struct_size; /* caller sets it; smaller is refused */
  uint64_t n_entries, n_accepted, n_nodes, n_sets; float ms_grid, ms_search, ms_components, ms_copy; } eg3d_polymatch_stats;
int eg3d_match_polylines_closeness(eg3d_ctx*, const eg3d_seeds* seeds /* NULL = the uploaded seeds */,
                                   uint32_t seed_begin, uint32_t seed_end, eg3d_polyline_matches* out, eg3d_polymatch_stats* stats);
void eg3d_free_polyline_matches(eg3d_polyline_matches*);

/* ---- pipeline 1: the polyline compatibility graph ------------------------------------------------------------------
 * The graph half of polyline_matching_similarity_graph (polyline_matcher.cpp:222-327), on the device; the community
 * detection the reference runs on the graph (Grappolo, third-party) is eg3d_detect_communities below, or a program of the
 * caller's: include/eg3d_host.h has both sides of its file seam. For every seed of [seed_begin, seed_end), ascending, the search of eg3d_match_polylines_closeness runs
 * at every entry of its track; ALL polylines within 10 px count (there is no acceptance rule). The distinct (view,
 * polyline) pairs of a point are a clique; nodes are numbered by first appearance, as the reference numbers them. A point
 * weighs (views with a close polyline) / (float)(pairs), 0 without any; the edge between (v1, p1) and (v2, p2) weighs
 * sum(weight over A and B) / sum(weight over A or B) with A = the points close to p1 on v1 whose track lists v2 and B = the
 * points close to p2 on v2 whose track lists v1, each sum a float that starts at 0 and adds in ascending point order; an
 * edge is kept where that is > 0. The cliques are expanded a fixed budget of edge keys at a time and merged into the
 * sorted list of distinct edges, so no input is refused for its size short of 2^31 distinct edges (EG3D_ERR_CAPACITY);
 * EG3D_SIMGRAPH_PAIR_BUDGET=n (read when the context is created; tests) sets the budget in keys.
 * An empty range, or no close polyline: n_nodes = 0, adj_off = {0}, EG3D_OK (the per-point and per-polyline arrays are
 * still there, all zero). A view id outside the rig, struct_size, seeds == NULL, the 10 px map and the threading rule: as
 * eg3d_match_polylines_closeness; the map is built by the first call of either and shared. */
typedef struct eg3d_simgraph {            /* library-owned; eg3d_free_simgraph */
  uint32_t n_nodes;      uint32_t* node_view;  uint32_t* node_pl;   /* polyline_matches_vector, in node-id order */
  uint32_t* adj_off;     /* [n_nodes + 1] adjacency_lists: both directions of every kept edge, neighbours ascending */
  uint32_t* adj_node;    float* adj_w;         /* [adj_off[n_nodes]] */
  uint32_t seed_begin;   uint32_t n_points;    /* = seed_end - seed_begin; point i is seed seed_begin + i */
  float* point_weight;   /* [n_points] */
  uint32_t* cp_off;      /* [n_points + 1] close_polylines, sparse: per point its (view, polyline) pairs, ascending */
  uint32_t* cp_view;     uint32_t* cp_pl;      /* [cp_off[n_points]] */
  uint32_t n_polylines;  /* = view_pl_off[n_views] */
  uint32_t* cr_off;      /* [n_polylines + 1] close_refpoints over the global polyline index view_pl_off[view] + pl */
  uint32_t* cr_point;    /* [cr_off[n_polylines]] absolute seed ids, ascending per row */
} eg3d_simgraph;
typedef struct eg3d_simgraph_stats { uint32_t struct_size; /* caller sets it; smaller is refused */
  uint64_t n_entries, n_nodes, n_edges /* undirected, kept */, n_pair_instances /* sum of m (m - 1) / 2 */, n_chunks;
  float ms_grid, ms_search /* count, scan, fill */, ms_graph /* lists, nodes, distinct edges */,
        ms_weights /* edge weights and the adjacency */, ms_copy; } eg3d_simgraph_stats;
int eg3d_similarity_graph(eg3d_ctx*, const eg3d_seeds* seeds /* NULL = the uploaded seeds */, uint32_t seed_begin,
                          uint32_t seed_end, eg3d_simgraph* out, eg3d_simgraph_stats* stats);
void eg3d_free_simgraph(eg3d_simgraph*);

/* ---- pipeline 1: community detection on the compatibility graph -----------------------------------------------------
 * A deterministic Louvain on the device (K11), in the place where the reference calls Grappolo. It keeps Grappolo's rules
 * (synchronous sweeps, equal gains go to the smaller label, two singletons do not swap, phases on the coarsened graph) and
 * uses exact arithmetic: a weight w is the integer llrint((double)w * 2^32), every sum is an integer sum, gains and the
 * modularity numerator N = (weight inside communities) * M - sum of a_c^2 (M = the sum of all directed weights, a_c = a
 * community's total degree) are exact 128-bit integers, and doubles appear only in the two threshold tests
 * (double)(N_new - N_old) < threshold * ((double)M * (double)M). The result does not depend on the device, the table size or
 * the order in which lanes arrive; tests/louvain_ref.py restates the algorithm and is its definition.
 * `g` is read for n_nodes, adj_off, adj_node and adj_w only (host memory): both directions of every edge, neighbours
 * strictly ascending, no self-loop, weights finite and in (0, 1], the two directions of an edge with the same weight bits,
 * fewer than 2^31 entries (EG3D_ERR_CAPACITY). A violation is EG3D_ERR_ARG (device-side check before anything else;
 * eg3d_last_error names the rule; `out` and `stats` stay untouched). ids[i] is the community of node i, numbered by
 * ascending smallest member; a node without a neighbour gets -1, which eg3d_host_sets_from_communities drops.
 * n_nodes == 0: an empty result, EG3D_OK. EG3D_LOUVAIN_TABLE_SLOTS=n (read when the context is created; tests) sets the
 * slots of the sweep's per-wavefront table (a power of two in 16 .. 1024, default 512); rows with more distinct
 * neighbouring communities than slots take the sort-and-reduce path (stats.n_overflow_rows). struct_size and the threading
 * rule: as eg3d_similarity_graph. */
typedef struct eg3d_louvain_params { uint32_t struct_size; /* caller sets it; smaller is refused */
  uint32_t max_phases /* 200 */, max_sweeps /* per phase: 1000 */;
  double sweep_threshold, phase_threshold /* 1e-6 each; negative or NaN is refused */; } eg3d_louvain_params; /* NULL = defaults; 0 in a field = its default */
typedef struct eg3d_communities { uint32_t n_nodes; int64_t* ids; uint32_t n_communities; } eg3d_communities; /* library-owned; eg3d_free_communities */
typedef struct eg3d_louvain_stats { uint32_t struct_size; /* caller sets it; smaller is refused */
  uint32_t n_phases, n_sweeps, n_communities, n_isolated; uint64_t n_overflow_rows /* summed over sweeps */,
  total_q /* M */, numer_hi, numer_lo /* the final N, two's complement */; double modularity /* (double)N / ((double)M * (double)M); 0 for M == 0 */;
  float ms_upload /* and the checks */, ms_sweeps, ms_coarsen /* renumbering and the coarse graphs */, ms_copy; } eg3d_louvain_stats;
int eg3d_detect_communities(eg3d_ctx*, const eg3d_simgraph* g, const eg3d_louvain_params* params, eg3d_communities* out,
                            eg3d_louvain_stats* stats);
void eg3d_free_communities(eg3d_communities*);

/* ---- fundamental matrices from the tracks, on the device (row N4, K12) ---------------------------------------------------
 * What generate_all_fundamental_matrices does before anything of the path can start: for every ORDERED pair of views the
 * points seen from both (ascending id; a repeated view id counts once; a point's position on a view is its LAST listed
 * observation with that id; entries with a view id outside [0, n_views) are ignored), and for pairs with at least 10 of
 * them a least-median-of-squares estimate over `iterations` normalised 8-point samples with a refit on the inliers. The
 * arithmetic is stated once, in csrc/eg3d_fund_core.h; include/eg3d_host.h's eg3d_host_estimate_fundamental is its plain
 * host form and the DEFINITION of the result: F, F_valid, n_common, n_pairs_failed and n_fits_degenerate of the two are
 * equal bit for bit, on any device, for any fit_budget and stage_points. (It is NOT the arithmetic of
 * eg3d_host_estimate_F to the bit: the normalisation takes sqrt(dx*dx + dy*dy) where that one calls hypot. Nor is it
 * OpenCV's LMedS, which is randomised: row N4 stays a documented non-parity.)
 * The call needs no context — F is part of the scene eg3d_create takes — makes its own stream and buffers on `device` and
 * frees all of them before it returns; the caller thread's current HIP device is the same after the call as before.
 * Outputs are the caller's: F [V][V][9] with the convention of eg3d_scene.F (l_j = F[i][j] x_i), F_valid [V][V], n_common [V][V] (may be NULL); a pair without a matrix has F = 0, F_valid = 0.
 * A pair with >= 10 common points whose every sample is degenerate (or has a non-finite median) counts in n_pairs_failed
 * and gets F_valid = 0; the call still returns EG3D_OK. The fits of `fit_budget` (pair, iteration)s are held on the device
 * at a time, in chunks of whole pairs (stats.n_chunks); the selection stages up to `stage_points` common points of a pair
 * in LDS and reads longer pairs from memory, to the same result.
 * EG3D_ERR_ARG (outputs and stats untouched): a struct_size smaller than the library's, n_views <= 0, seeds / F / F_valid
 * NULL, a NULL track array with n_seeds > 0, trk_off not ascending from 0. EG3D_ERR_CAPACITY: more than 8192 views.
 * EG3D_ERR_NODEVICE / EG3D_ERR_HIP as elsewhere. Any caller thread; concurrent calls are independent. */
typedef struct eg3d_fund_params { uint32_t struct_size; /* caller sets it; smaller is refused */
  uint32_t iterations /* 0 = 300 */; uint64_t rng_seed;
  uint32_t fit_budget   /* fits held on the device at a time; 0 = default (2^20); raised to one pair's worth */;
  uint32_t stage_points /* common points of a pair staged in LDS; 0 = default (1024, at most 4096); longer pairs are read from memory */;
} eg3d_fund_params; /* NULL = defaults */
typedef struct eg3d_fund_stats { uint32_t struct_size; /* caller sets it; smaller is refused */
  uint32_t n_pairs_valid /* ordered pairs with a matrix */, n_pairs_failed, n_chunks /* 0 on the host */;
  uint64_t n_common_total /* over the ordered pairs with >= 10 */, n_fits /* sample fits: those pairs x iterations */,
  n_fits_degenerate /* of the sample fits */, n_exact_medians /* device only: medians the selection had to compute exactly */;
  float ms_upload, ms_lists, ms_samples, ms_fits, ms_select /* with the inliers and the refit's normal matrix */,
  ms_refit /* its solve and its median test */, ms_copy; } eg3d_fund_stats;
int eg3d_estimate_fundamental(int device, int32_t n_views, const eg3d_seeds* seeds, const eg3d_fund_params* params /* NULL = defaults */,
                              double* F /* [V][V][9] */, uint8_t* F_valid /* [V][V] */, uint32_t* n_common /* [V][V], may be NULL */,
                              eg3d_fund_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* EG3D_H_ */
