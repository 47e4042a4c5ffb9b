// eg3d_k3_chains.hip — gfx950 kernels of stage B up to the finished chains: tasks -> hypotheses -> chain seeds -> chains.
//   k_task_setup      1 lane / task         3-view selection, hypothesis count
//   k3a_orient, k3a_follow_spec  1 lane / hypothesis, 1 lane / list — the wave SERVES its lanes' triangulation requests
//                                           densely from 64 slots in LDS (eg3d_k3a_engine.h)
//   k3s_select        1 lane / task         uniqueness rule -> chain seeds
//   k3b_expand        1 WAVE / chain        expand-all-views (wave-cooperative Gauss-Newton; eg3d_k3b_expand.h)
//   k3c_engine        1 LANE / chain        the second, slower form of the expand stage (eg3d_k3c_engine.h; builds with
//                                           -DEG3D_WITH_K3C_ENGINE only)
// All arithmetic follows the contract in DESIGN.md (no FMA contraction: -ffp-contract=off).
//
// K3a and K3b (and K3c) share this ONE translation unit on purpose. The timing builds (-DEG3D_SECTION_TIMING,
// EG3D_GN_COUNTERS) make both kernels add into the one __device__ g_gn_dbg[128] of eg3d_dev_coopgn.h, and gn_dbg_read below
// reads it. The project builds with -fno-gpu-rdc: a __device__ variable belongs to exactly one translation unit, so in two
// units each kernel would add into a counter block of its own and gn_dbg_read would see one of them. The same holds for
// g_k3c_dbg / g_k3c_prof of eg3d_k3c_engine.h and k3c_dbg_read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_pipeline.h"
#include "eg3d_dev_coopgn.h"
#include "eg3d_kernels.h"

// ------------------------------------------------------------------ K3a --------
// Hypothesis evaluation: eg3d_k3a_engine.h (k3a_orient, k3a_follow_spec); what it computes is stated sequentially by
// evaluate_hypothesis in eg3d_dev_follow.h (the host simulation of the tests runs that).
#ifndef EG3D_K3A_WAVES
#define EG3D_K3A_WAVES 2 /* waves/SIMD the register allocation of K3a aims at: 256 VGPRs, nothing spills (at 3: 168 VGPRs,
                            86-102 spilled; same speed on C3', K3a 1.50 -> 1.30 ms on C2, half the L2<->fabric traffic) */
#endif
// (which hypotheses are compatible is decided where it is asked, by k3s_select: hyp_compatible in eg3d_dev_follow.h)
#include "eg3d_k3a_engine.h"
// ------------------------------------------------------------------ K3b --------
// The expand stage: eg3d_k3b_expand.h (k3b_expand_t, k_pool_init, k_collect_overflow, k_chain_cost).
#include "eg3d_k3b_expand.h"
// The lane-per-chain engine is a second, slower form of the expand stage: compiled only into builds made with
// -DEG3D_WITH_K3C_ENGINE (edgegraph3d_amd/build.py build_hip_engine -> variants/libeg3d_engine.so); the product libraries
// do not carry it. Its state machine (eg3d_chain_sm.h) stays checked on the host by tests/hostsim.
#ifdef EG3D_WITH_K3C_ENGINE
#include "eg3d_k3c_engine.h"
#endif

namespace eg3d {

// ------------------------------------------------------------------ tasks ------
__global__ void k_task_setup(StageAView a, const int32_t* map_view, const uint32_t* map_entry, const uint32_t* map_n,
                             TaskDesc* tasks, uint32_t* n_hyp) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n_tasks) return;
  TaskDesc d;
  task_setup(a, t, map_view, map_entry, map_n, d);
  tasks[t] = d;
  n_hyp[t] = d.n_hyp;
}
void launch_task_setup(hipStream_t st, StageAView a, const int32_t* map_view, const uint32_t* map_entry,
                       const uint32_t* map_n, TaskDesc* tasks, uint32_t* n_hyp) {
  if (!a.n_tasks) return;
  hipLaunchKernelGGL(k_task_setup, blocks_for(a.n_tasks, 256), dim3(256), 0, st, a, map_view, map_entry, map_n, tasks,
                     n_hyp);
}

// K3a as a request/serve engine (eg3d_k3a_engine.h): one wavefront per block
void launch_k3a_engine(hipStream_t st, uint32_t orient_waves, uint32_t follow_waves, uint32_t lanes_per_wave, DevScene s,
                       StageAView a, const TaskDesc* tasks, const uint32_t* hyp_off, uint32_t n_hyp, HypResult* res,
                       HPoint* follow_scratch, uint32_t hyp_cap, HPoint* arena, uint32_t arena_cap, Counters* ctr,
                       uint32_t* queue3, uint32_t* items) {
  if (!n_hyp) return;
  hipLaunchKernelGGL(k3a_orient, dim3(orient_waves), dim3(64), 0, st, s, a, tasks, hyp_off, n_hyp, res, hyp_cap, arena,
                     arena_cap, ctr, queue3, lanes_per_wave, items, queue3 + 2);
  hipLaunchKernelGGL(k3a_follow_spec, dim3(follow_waves), dim3(64), 0, st, s, res, follow_scratch, hyp_cap, arena, arena_cap, ctr, queue3 + 1, lanes_per_wave, items, queue3 + 2);
}

// ------------------------------------------------------------------ K3s --------
__global__ void k3s_select(uint32_t n_tasks, const uint32_t* hyp_off, const HypResult* res, ChainSeed* seeds_out,
                           uint32_t* valid) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tasks) return;
  ChainSeed cs;
  cs.task = t;
  cs.winner = 0;
  cs.pts2_src = 0xffffffffu;
  cs.n1 = 0;
  cs.n2 = 0;
  bool ok = false;
  if (hyp_off[t + 1] > hyp_off[t]) ok = select_task(res, hyp_off[t], hyp_off[t + 1], cs);
  seeds_out[t] = cs;
  valid[t] = ok ? 1u : 0u;
}
__global__ void k_compact_chains(uint32_t n_tasks, const ChainSeed* per_task, const uint32_t* valid,
                                 const uint32_t* chain_off, ChainSeed* chains) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tasks) return;
  if (valid[t]) chains[chain_off[t]] = per_task[t];
}
void launch_k3s(hipStream_t st, uint32_t n_tasks, const uint32_t* hyp_off, const HypResult* res, ChainSeed* per_task,
                uint32_t* valid) {
  if (!n_tasks) return;
  hipLaunchKernelGGL(k3s_select, blocks_for(n_tasks, 256), dim3(256), 0, st, n_tasks, hyp_off, res, per_task, valid);
}
void launch_compact_chains(hipStream_t st, uint32_t n_tasks, const ChainSeed* per_task, const uint32_t* valid,
                           const uint32_t* chain_off, ChainSeed* chains) {
  if (!n_tasks) return;
  hipLaunchKernelGGL(k_compact_chains, blocks_for(n_tasks, 256), dim3(256), 0, st, n_tasks, per_task, valid, chain_off,
                     chains);
}

#ifdef EG3D_GN_COUNTERS
int gn_dbg_read(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gn_dbg), sizeof(unsigned long long) * 128) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[128] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_gn_dbg), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

// ------------------------------------------------------------------ K3b --------
// Three instantiations (round 4), see TeamWaveT: small scenes (50.6 k -> 45 k instructions, 116 instead of 262 spilled
// vector registers), general, many views.
static_assert(EG3D_STAGE_VTX_HOST == EG3D_STAGE_VTX, "the host's small-scene rule must match the side walks' staging capacity");
static_assert(EG3D_GN_PACK_MAX >= EG3D_SMALL_SCENE_VIEWS_HOST, "a small scene's solves must fit a packed round");
static_assert(2 * EG3D_SMALL_SCENE_VIEWS_HOST + 8 <= EG3D_COOP_ROWS && 2 * (EG3D_SMALL_SCENE_VIEWS_HOST + 1) + 8 > EG3D_COOP_ROWS,
              "EG3D_SMALL_SCENE_VIEWS_HOST must be the last view count whose N-view step lists fit LDS");
static constexpr auto k3b_expand_small = k3b_expand_t<EG3D_K3B_WAVES, 0, 0>;
static constexpr auto k3b_expand = k3b_expand_t<EG3D_K3B_WAVES, 0, 1>;
#ifndef EG3D_MANY_WAVES
#define EG3D_MANY_WAVES EG3D_K3B_WAVES /* waves per SIMD of the many-views build (fewer = more registers for kept chunks) */
#endif
static constexpr auto k3b_expand_many = k3b_expand_t<EG3D_MANY_WAVES, EG3D_MANY_KEEP, 2>;
int k3b_blocks_per_cu() {  // the largest residency of the builds sizes the slot pools
  int best = 0;
  for (int k = 0; k < 3; k++) {
    int n = 0;
    const void* f = k == 0 ? (const void*)k3b_expand_small : k == 1 ? (const void*)k3b_expand : (const void*)k3b_expand_many;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, 64, 0) != hipSuccess || n < 1) return 0;
    best = n > best ? n : best;
  }
  return best;
}
void launch_pool_init(hipStream_t st, SlotPools pools) {
  hipLaunchKernelGGL(k_pool_init, dim3(8), dim3(256), 0, st, pools);
}
void launch_chain_cost(hipStream_t st, StageAView a, const TaskDesc* tasks, const ChainSeed* chains, uint32_t n_chains,
                       uint32_t* cost, uint32_t* idx) {
  if (!n_chains) return;
  hipLaunchKernelGGL(k_chain_cost, blocks_for(n_chains, 256), dim3(256), 0, st, a, tasks, chains, n_chains, cost, idx);
}
void launch_k3b(hipStream_t st, DevScene s, StageAView a, const TaskDesc* tasks, const ChainSeed* chains,
                uint32_t n_chains, const uint32_t* hyp_off, const HypResult* res, const HPoint* arena,
                const int32_t* map_view, const uint32_t* map_entry, const uint32_t* map_n, ChainLayout L,
                unsigned char* slices, SlotPools pools, StageBuf stage, ChainOut* outs, uint32_t* out_points,
                uint32_t* out_obs, Counters* ctr, const uint32_t* order, int scene_class) {
  if (!n_chains) return;
  if (scene_class == 0)
    hipLaunchKernelGGL(k3b_expand_small, dim3(n_chains), dim3(64), 0, st, s, a, tasks, chains, n_chains, hyp_off, res,
                       arena, map_view, map_entry, map_n, L, slices, pools, stage, outs, out_points, out_obs, ctr, order);
  else if (scene_class == 2)
    hipLaunchKernelGGL(k3b_expand_many, dim3(n_chains), dim3(64), 0, st, s, a, tasks, chains, n_chains, hyp_off, res,
                       arena, map_view, map_entry, map_n, L, slices, pools, stage, outs, out_points, out_obs, ctr, order);
  else
    hipLaunchKernelGGL(k3b_expand, dim3(n_chains), dim3(64), 0, st, s, a, tasks, chains, n_chains, hyp_off, res,
                       arena, map_view, map_entry, map_n, L, slices, pools, stage, outs, out_points, out_obs, ctr, order);
}
void launch_collect_overflow(hipStream_t st, const ChainOut* outs, const uint32_t* order, uint32_t n, uint32_t* redo,
                             uint32_t* n_redo, Counters* ctr) {
  if (!n) return;
  hipLaunchKernelGGL(k_collect_overflow, blocks_for(n, 256), dim3(256), 0, st, outs, order, n, redo, n_redo, ctr);
}

#ifdef EG3D_WITH_K3C_ENGINE
// ------------------------------------------------------------------ K3c --------
// The expand stage as a lane-per-chain engine (eg3d_k3c_engine.h): n_waves single-wavefront blocks whose first
// lanes_per_wave lanes each own a working slice (slices: [n_waves * lanes_per_wave] x L.total bytes) and take chains from
// the launch's queue (*queue zeroed by the caller) until it is empty. long_gn = 0: scenes whose solves all fit a packed
// round of the solver (<= 32 rows); a longer request raises CTR_LONG_REFUSED and the host repeats the launch with 1.
static constexpr auto k3c_engine_short = k3c_engine_t<false>;
static constexpr auto k3c_engine_long = k3c_engine_t<true>;
int k3c_blocks_per_cu() {
  int a = 0, b = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, (const void*)k3c_engine_short, 64, 0) != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, (const void*)k3c_engine_long, 64, 0) != hipSuccess) return 0;
  return a < b ? a : b;
}
void launch_k3c(hipStream_t st, uint32_t n_waves, uint32_t lanes_per_wave, DevScene s, StageAView a, const TaskDesc* tasks,
                const ChainSeed* chains, uint32_t n_chains, const uint32_t* hyp_off, const HypResult* res, const HPoint* arena,
                const int32_t* map_view, const uint32_t* map_entry, const uint32_t* map_n, ChainLayout L, unsigned char* slices,
                StageBuf stage, ChainOut* outs, uint32_t* out_points, uint32_t* out_obs, Counters* ctr, const uint32_t* order,
                uint32_t* queue, int long_gn) {
  if (!n_chains) return;
  if (long_gn)
    hipLaunchKernelGGL(k3c_engine_long, dim3(n_waves), dim3(64), 0, st, s, a, tasks, chains, n_chains, hyp_off, res, arena,
                       map_view, map_entry, map_n, L, slices, stage, outs, out_points, out_obs, ctr, order, queue, lanes_per_wave);
  else
    hipLaunchKernelGGL(k3c_engine_short, dim3(n_waves), dim3(64), 0, st, s, a, tasks, chains, n_chains, hyp_off, res, arena,
                       map_view, map_entry, map_n, L, slices, stage, outs, out_points, out_obs, ctr, order, queue, lanes_per_wave);
}
#if defined(EG3D_SECTION_TIMING) || defined(EG3D_K3C_TIMING)
int k3c_dbg_read(unsigned long long* out, int reset) {  // out[128]: g_k3c_dbg[32] then g_k3c_prof[96]
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_k3c_dbg), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out + 32, HIP_SYMBOL(g_k3c_prof), sizeof(unsigned long long) * 96) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[96] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_k3c_dbg), z, sizeof(unsigned long long) * 32) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_k3c_prof), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
#endif  // EG3D_WITH_K3C_ENGINE

}  // namespace eg3d
