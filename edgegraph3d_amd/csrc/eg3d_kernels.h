// Host-visible declarations of the kernel launch wrappers and the types they share, one section per eg3d_k*.hip file of
// stages K0-K7 (the later stages K8-K12 have headers of their own, which include this one).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_pipeline.h"
#include "eg3d_matched_core.h"

namespace eg3d {

// ---- shared by the stages ----
struct SeedsDev {
  const uint32_t* trk_off;
  const int32_t* trk_view;
  const float* trk_xy;
};

// Observation of `seed` in view `view`: the LAST track entry with that view id (Q2).
__device__ __forceinline__ void seed_obs_in_view(const SeedsDev& sd, uint32_t t0, uint32_t k, int32_t view, float& x,
                                                 float& y) {
  x = 0.f;
  y = 0.f;
  for (uint32_t i = 0; i < k; i++)
    if (sd.trk_view[t0 + i] == view) {
      x = sd.trk_xy[2 * (t0 + i)];
      y = sd.trk_xy[2 * (t0 + i) + 1];
    }
}

enum : uint32_t { CTR_ARENA_OVERFLOW = 0x100u, CTR_SLOT_STARVED = 0x200u /* k3b_expand found no free working slice (internal) */,
                  CTR_LONG_REFUSED = 0x400u /* the few-views build of k3b_expand met a solve of more than 32 rows (internal) */,
                  CTR_N1_NO_PROGRESS = 0x800u /* k_n1_samples<., true>: a jump past a held interval did not advance (internal) */ };
typedef uint64_t eg3d_off_t;  // element type of obs_off in the output cloud (include/eg3d.h)
struct Counters {
  uint32_t arena_used;
  uint32_t flags;  // EG3D_FLAG_* bits | CTR_ARENA_OVERFLOW
  unsigned long long bytes;  // algorithmic bytes of polyline vertices touched
  uint32_t max_chain_ticks;  // k3b_expand: the longest time one chain held its wavefront (ticks of the constant-rate clock, wall_clock64)
  uint32_t pad_;
  unsigned long long hits_used;  // k2_epipolar_hits: the cursor the tasks claim their region of the hits from
  // K3a walk service (eg3d_k3a_engine.h): walks the wave finished for a lane, and the 64-segment passes that took; every
  // wavefront adds its totals once, at exit (read by eg3d_probe_k3a_walks in the test-only builds)
  uint32_t k3a_walks_served;
  uint32_t k3a_walk_passes;
};
// grid of a launch with one lane (or one wave's worth of lanes) per item: ceil(n / per_block) blocks
inline dim3 blocks_for(uint64_t n, uint32_t per_block) { return dim3((unsigned)((n + per_block - 1) / per_block)); }

// ---- eg3d_k_util.hip ----
// arguments of k_publish: up to 6 runs of device words copied to the host mailbox, words cleared afterwards
struct PubArgs {
  const uint32_t* src[6];
  uint32_t words[6];
  uint32_t* clear[3];
  int n, n_clear;
};
enum { EG3D_MBOX_WORDS = 64 };
void launch_publish(hipStream_t st, const PubArgs& a, uint32_t* mbox_dev, uint32_t seq);
// {out[n], 1 if the scan wrapped} -> total_and_flag[0..1] (flag word must be zero before the launch)
void launch_scan_check(hipStream_t st, const uint32_t* out, uint64_t n_plus_one, uint32_t* wrapped);

// ---- eg3d_k0_grid.hip ----
#define EG3D_K0_PL_BITS_HOST 19 /* = EG3D_K0_PL_BITS (static_assert in eg3d_k0_grid.hip) */
// K0: the uniform grids on the device. fill = false counts the (cell, polyline) pairs of every polyline
// into cnt[g]; fill = true writes them as 64-bit keys (view * cells + cell) << 19 | polyline behind off[g].
void launch_k0_pairs(hipStream_t st, bool fill, DevScene s, uint32_t n_pl, float cell_dim, int map_w, int map_h, uint32_t* cnt,
                     const uint32_t* off, unsigned long long* keys, uint32_t* dropped);
void launch_k0_csr(hipStream_t st, const unsigned long long* keys, uint32_t n, uint32_t total_cells, uint32_t* off, uint32_t* ids);

// ---- eg3d_k1_k2_refpoints.hip ----
void launch_seed_prep(hipStream_t st, SeedsDev sd, uint32_t seed_begin, uint32_t n_seeds, uint32_t sv_base,
                      uint32_t* sv_seed, int32_t* map_view, uint32_t* map_entry, uint32_t* map_n);
void launch_k1_count_raw(hipStream_t st, DevScene s, SeedsDev sd, uint32_t sv_base, uint32_t n_sv, const uint32_t* sv_seed,
                         uint32_t* raw_cnt);
void launch_k1(hipStream_t st, DevScene s, SeedsDev sd, uint32_t sv_base, uint32_t n_sv, const uint32_t* sv_seed,
               const uint32_t* raw_off, uint32_t* cand_pl, Obs* start_hits, uint32_t* cand_cnt, uint32_t* start_cnt,
               uint32_t* sv_vtx);
void launch_task_fill(hipStream_t st, SeedsDev sd, uint32_t sv_base, uint32_t n_sv, const uint32_t* sv_seed,
                      const uint32_t* start_cnt, const uint32_t* task_off, uint32_t* task_seed, uint32_t* task_entry,
                      uint32_t* task_hit, uint32_t* task_k, const uint32_t* sv_vtx, Counters* ctr);
// K2 in one pass: one wavefront per task stages the task's hits in LDS (stage_cap <= EG3D_K2_STAGE_MAX per
// wave), claims its region of `hits` from ctr->hits_used (zeroed by the caller) and writes list_cnt, list_ptr and the hits.
// ctr->hits_used > hits_cap afterwards: `hits` was too small and is incomplete; enlarge it and launch again.
#define EG3D_K2_STAGE_MAX 128u
void launch_k2(hipStream_t st, DevScene s, SeedsDev sd, uint32_t sv_base, uint32_t n_tasks, const uint32_t* task_seed,
               const uint32_t* task_entry, const uint32_t* task_hit, const uint32_t* task_list_off, const uint32_t* raw_off,
               const uint32_t* cand_pl, const uint32_t* cand_cnt, const Obs* start_hits, uint32_t* list_cnt, uint32_t* list_ptr,
               Obs* hits, uint32_t hits_cap, uint32_t stage_cap, Counters* ctr);

// ---- eg3d_n1_sets.hip: pipelines 1-2 extractor, sets of potentially compatible polylines -> tasks ----
// CSR over rows (set * V + view) of view-local polyline ids, ascending per row (device copies).
struct SetsDev {
  uint32_t n_views;
  const uint32_t* row_off;  // [n_sets * V + 1]
  const uint32_t* pl_ids;
};
// items = entries [item_begin, item_begin + n_items) of pl_ids; fill=false counts the 20 px samples
// of each item's polyline, fill=true writes them (one task per sample) at sample_off[item]
void launch_n1_samples(hipStream_t st, bool fill, DevScene s, SetsDev sets, uint32_t n_rows, uint32_t item_begin,
                       uint32_t n_items, uint32_t* sample_cnt, const uint32_t* sample_off, Obs* samples,
                       uint32_t* task_seed, uint32_t* task_entry, uint32_t* task_hit, uint32_t* task_list_off,
                       uint32_t* task_row0, Counters* ctr, const IvTable* matched = nullptr, uint32_t* skip_cnt = nullptr);
// one wavefront per (task, view): hits of the sample's epipolar line on the set's polylines of that view
void launch_n1_hits(hipStream_t st, bool fill, DevScene s, SetsDev sets, uint32_t n_tasks, const Obs* samples,
                    const uint32_t* task_row0, uint32_t* list_cnt, const uint32_t* list_ptr, Obs* hits, Counters* ctr,
                    const IvTable* matched = nullptr, uint32_t* drop_cnt = nullptr);
// `matched` (device pointers, checked by launch_n1_check_intervals) selects the MATCHED instantiations of both kernels:
// samples and hits inside a held interval are left out (eg3d_matched_core.h). The count passes (fill = false) write, when
// the pointer is given, skip_cnt[item] = samples skipped and drop_cnt[task] = hits dropped.
// *bad (zeroed by the caller) becomes non-zero when a row of the table fails check_interval_row; total = iv.off[n_pl]
void launch_n1_check_intervals(hipStream_t st, DevScene s, IvTable iv, uint64_t total, uint32_t n_pl, uint32_t* bad);

// ---- eg3d_k3_chains.hip ----
void launch_task_setup(hipStream_t st, StageAView a, const int32_t* map_view, const uint32_t* map_entry,
                       const uint32_t* map_n, TaskDesc* tasks, uint32_t* n_hyp);
// K3a as a request/serve engine (eg3d_k3a_engine.h): orient_waves / follow_waves single-wavefront blocks, of which
// the first lanes_per_wave lanes take work; follow_scratch: min(hyp_cap, EG3D_K3A_STAGE_POINTS) HPoints per lane of
// follow_waves x 64; queue3: three
// zeroed counters (hypotheses taken, lists taken, lists to follow); items: 2 x n_hyp words (the lists to follow)
#define EG3D_K3A_STAGE_POINTS 16u /* = EG3D_K3A_STAGE of eg3d_k3a_engine.h */
void launch_k3a_engine(hipStream_t st, uint32_t orient_waves, uint32_t follow_waves, uint32_t lanes_per_wave, DevScene s,
                       StageAView a, const TaskDesc* tasks, const uint32_t* hyp_off, uint32_t n_hyp, HypResult* res,
                       HPoint* follow_scratch, uint32_t hyp_cap, HPoint* arena, uint32_t arena_cap, Counters* ctr,
                       uint32_t* queue3, uint32_t* items);
void launch_k3s(hipStream_t st, uint32_t n_tasks, const uint32_t* hyp_off, const HypResult* res, ChainSeed* per_task,
                uint32_t* valid);
void launch_compact_chains(hipStream_t st, uint32_t n_tasks, const ChainSeed* per_task, const uint32_t* valid,
                           const uint32_t* chain_off, ChainSeed* chains);
// Pools of working-slice slots of k3b_expand, one per XCD (see the kernel): 8 x `stride` words,
// [0] pop tickets, [16] push tickets, [32 ..] a ring of ring_n (power of two >= slots_per_xcd) cells.
struct SlotPools {
  uint32_t* base;
  uint32_t stride, ring_n, slots_per_xcd;
};
#define EG3D_SMALL_SCENE_VIEWS_HOST 28 /* the last view count whose N-view step lists fit LDS (2 V + 8 <= 64; static_assert in eg3d_k3_chains.hip) */
#define EG3D_STAGE_VTX_HOST 512 /* = EG3D_STAGE_VTX: vertices of a polyline the side walks stage in LDS */
int k3b_blocks_per_cu();  // resident k3b_expand workgroups per CU (occupancy query; 0 on failure)
void launch_pool_init(hipStream_t st, SlotPools pools);
void launch_chain_cost(hipStream_t st, StageAView a, const TaskDesc* tasks, const ChainSeed* chains, uint32_t n_chains,
                       uint32_t* cost, uint32_t* idx);
void launch_k3b(hipStream_t st, DevScene s, StageAView a, const TaskDesc* tasks, const ChainSeed* chains,
                uint32_t n_chains, const uint32_t* hyp_off, const HypResult* res, const HPoint* arena,
                const int32_t* map_view, const uint32_t* map_entry, const uint32_t* map_n, ChainLayout L,
                unsigned char* slices, SlotPools pools, StageBuf stage, ChainOut* outs, uint32_t* out_points,
                uint32_t* out_obs, Counters* ctr, const uint32_t* order, int scene_class /* polylines of <= 512 vertices: 0 small (<= 28 views) or 2 many views (>= 29); 1 general: the build of the kernel without the paths such a scene cannot reach */);
void launch_collect_overflow(hipStream_t st, const ChainOut* outs, const uint32_t* order, uint32_t n, uint32_t* redo,
                             uint32_t* n_redo, Counters* ctr);
// lane-per-chain engine of the expand stage (eg3d_k3c_engine.h; builds with -DEG3D_WITH_K3C_ENGINE only)
#ifdef EG3D_WITH_K3C_ENGINE
int k3c_blocks_per_cu();
void launch_k3c(hipStream_t st, uint32_t n_waves, uint32_t lanes_per_wave, DevScene s, StageAView a, const TaskDesc* tasks,
                const ChainSeed* chains, uint32_t n_chains, const uint32_t* hyp_off, const HypResult* res, const HPoint* arena,
                const int32_t* map_view, const uint32_t* map_entry, const uint32_t* map_n, ChainLayout L, unsigned char* slices,
                StageBuf stage, ChainOut* outs, uint32_t* out_points, uint32_t* out_obs, Counters* ctr, const uint32_t* order,
                uint32_t* queue, int long_gn);
#endif

// ---- eg3d_k4_emit.hip ----
void launch_k4(hipStream_t st, const TaskDesc* tasks, const ChainSeed* chains, uint32_t n_chains, StageBuf stage,
               const ChainOut* outs, const uint32_t* point_off, const uint32_t* obs_off_in, uint64_t point_base,
               uint64_t obs_base, uint32_t key0_base, float* X, eg3d_off_t* obs_off, int32_t* obs_view, uint32_t* obs_pl,
               uint32_t* obs_seg, float* obs_xy, uint32_t* key);

// ---- eg3d_k5_filter.hip: the FP32 Gauss-Newton filter on host clouds (eg3d_gn_filter) and on device-resident ones
// (eg3d_gn_filter_device) ----
void launch_k5(hipStream_t st, const float* cam_P, int n_views, const float* X, const uint32_t* obs_off,
               const int32_t* obs_view, const float* obs_xy, uint64_t n, float gn_max_mse, int legacy_abs, float* X_out,
               uint8_t* inlier);
// Second instantiation of the K5 body: 64-bit offsets without a sentinel, optional keep mask, histogram of the inliers'
// list lengths, device-side checks of what the host form validates on the host (see k5_gn_filter).
enum : uint32_t { K5_FLAG_BAD_VIEW = 1u /* a view id outside [0, n_views) */,
                  K5_FLAG_BAD_OFFSETS = 2u /* a list that is not an ascending range inside [0, n_obs], or longer than K5_MAX_LIST */ };
#define K5_MAX_LIST (1u << 24) /* observations of ONE point on the device-cloud entry points: 64 such lists sum to at most 2^30, inside the int of wave_incl_scan */
struct K5Host {};  // eg3d_gn_filter: nothing beyond the legacy arguments
struct K5Dev {
  const uint8_t* keep;       // may be null: all points
  uint64_t n_obs;            // end of the last point's list
  unsigned long long* hist;  // [n_views + 2], zeroed by the caller
  uint32_t* flags;           // K5_FLAG_*, zeroed by the caller
};
template <bool SENTINEL>
struct K5ExtOf { typedef K5Dev type; };
template <>
struct K5ExtOf<true> { typedef K5Host type; };
template <bool SENTINEL>
using K5Ext = typename K5ExtOf<SENTINEL>::type;
void launch_k5_device(hipStream_t st, const float* cam_P, int n_views, const float* X, const eg3d_off_t* obs_off,
                      const int32_t* obs_view, const float* obs_xy, uint64_t n, float gn_max_mse, int legacy_abs, float* X_out,
                      uint8_t* inlier, K5Dev ext);

// ---- eg3d_k6_compact.hip: the compaction of a device-resident cloud (eg3d_compact_device) ----
// Order-preserving stream compaction of a device cloud, three launches. A point survives when keep[i] != 0 (keep may be
// null) and its list is longer than min_obs (min_obs < 0: no count test).
struct CloudView {  // = eg3d_device_edgepoints without `complete`
  uint64_t n_points, n_obs;
  const float* X;
  const eg3d_off_t* obs_off;
  const int32_t* obs_view;
  const uint32_t* obs_pl;
  const uint32_t* obs_seg;
  const float* obs_xy;
  const uint32_t* key;
};
struct CloudOut {
  float* X;
  eg3d_off_t* obs_off;
  int32_t* obs_view;
  uint32_t* obs_pl;
  uint32_t* obs_seg;
  float* obs_xy;
  uint32_t* key;
};
#define K6_BLOCK 256
// (1) per K6_BLOCK source points: surviving points and observations -> blk[2 b], blk[2 b + 1]
void launch_compact_count(hipStream_t st, CloudView in, const uint8_t* keep, int32_t min_obs, unsigned long long* blk,
                          uint32_t* flags);
// (2) exclusive scan of both columns in place, totals -> blk[2 n_blocks], blk[2 n_blocks + 1]
void launch_compact_scan(hipStream_t st, uint64_t n_blocks, unsigned long long* blk);
// (3) scatter; nt: non-temporal loads of the source
void launch_compact_scatter(hipStream_t st, CloudView in, const uint8_t* keep, const float* X_new, int32_t min_obs,
                            const unsigned long long* blk, CloudOut out, bool nt);

// ---- eg3d_k7_dedup.hip: the 3 px de-duplication of a device-resident cloud (eg3d_dedup_device) ----
// The claim map: per view a w x h grid of 3 px cells, w = ceil((float)width / 3), h = ceil((float)height / 3) as the host
// step computes them; an entry is the smallest point index that has an observation in the cell, 0xFFFFFFFF = none yet.
struct K7Map {
  uint32_t* first;  // [n_views][h][w]
  int32_t n_views, w, h;
};
#define K7_BLOCK 256
#define K7_UNCLAIMED 0xFFFFFFFFu
// (1) one lane per observation: atomicMin(first[cell], index_base + owning point)
void launch_dedup_claim(hipStream_t st, CloudView in, K7Map m, uint32_t index_base);
// (2) 8 lanes per point: keep[i] = an observation of i lies in a cell that holds index_base + i; *n_kept += kept points;
//     K5_FLAG_BAD_OFFSETS into *flags for offsets that do not ascend within [0, n_obs]
void launch_dedup_keep(hipStream_t st, CloudView in, K7Map m, uint32_t index_base, uint8_t* keep, unsigned long long* n_kept,
                       uint32_t* flags);

// ---- eg3d_k7b_claims.hip: what the dedup in phases adds (include/eg3d_dedup_phases.h) ----
#define K7B_BLOCK 256
#define K7B_MAX_BLOCKS 2048 /* of k7_claims_min: maps of more than 2 097 152 cells go round by grid stride */
// first[c] = min(first[c], other[c]) for c < n; *n_lowered += the entries that got smaller. `first` must be 16-byte aligned
// (a context's map is); `other` needs 4-byte alignment only and is never written; write_all: the form that writes every word back (measured against the default, which
// writes only the words it lowered)
void launch_claims_min(hipStream_t st, uint32_t* first, const uint32_t* other, uint64_t n, unsigned long long* n_lowered,
                       bool write_all);
// one lane per point: K5_FLAG_BAD_OFFSETS into *flags for offsets that do not ascend within [0, n_obs]
void launch_offsets_check(hipStream_t st, CloudView in, uint32_t* flags);

}  // namespace eg3d
