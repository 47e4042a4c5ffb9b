// eg3d_k4_emit.hip — K4 (gfx950):
//   k4_emit           1 WAVE / chain        ordered SoA output (wave prefix sum of obs counts, flat coalesced copy)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_pipeline.h"
#include "eg3d_dev_coopgn.h"
#include "eg3d_kernels.h"

namespace eg3d {

// ------------------------------------------------------------------ K4 ---------
// One wavefront per chain, in OUTPUT order: the chain's packed record (k3b_expand) becomes its slice
// of the ordered SoA cloud. Lanes take consecutive points; the observation offset of each point is
// the chain's base plus a wave prefix sum of the per-point counts; the observations of the record are
// already one flat range, so lane f copies observation f: coalesced 16-byte reads, coalesced rows in
// every output array.
__global__ void __launch_bounds__(64) k4_emit(const TaskDesc* tasks, const ChainSeed* chains, uint32_t n_chains,
                                              StageBuf stage, const ChainOut* outs, const uint32_t* point_off,
                                              const uint32_t* obs_off_in, uint64_t point_base, uint64_t obs_base,
                                              uint32_t key0_base, float* X, eg3d_off_t* obs_off, int32_t* obs_view,
                                              uint32_t* obs_pl, uint32_t* obs_seg, float* obs_xy, uint32_t* key) {
  const uint32_t j = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const ChainOut co = outs[j];
  const StagePt* spt = stage.pts + co.spt;
  const Obs* sob = stage.obs + co.sobs;
  const TaskDesc d = tasks[chains[j].task];
  const uint64_t pbase = point_base + point_off[j];
  const uint64_t obase = obs_base + obs_off_in[j];
  uint32_t run = 0;  // observations of the points before this group of 64
  for (uint32_t i0 = 0; i0 < co.n_points; i0 += 64) {
    const uint32_t i = i0 + lane;
    const bool act = i < co.n_points;
    StagePt p;
    p.nobs = 0;
    p.X[0] = p.X[1] = p.X[2] = 0.f;
    if (act) p = spt[i];
    const uint32_t incl = (uint32_t)wave_incl_scan((int)p.nobs);  // inclusive wave scan of the observation counts
    const uint32_t total = lane_bcast(incl, 63);
    if (act) {
      const uint64_t pi = pbase + i;
      X[3 * pi] = p.X[0];
      X[3 * pi + 1] = p.X[1];
      X[3 * pi + 2] = p.X[2];
      obs_off[pi] = (eg3d_off_t)(obase + run + (incl - p.nobs));
      key[4 * pi] = d.seed + key0_base;
      key[4 * pi + 1] = d.entry;
      key[4 * pi + 2] = d.hit;
      key[4 * pi + 3] = i;
    }
    run += total;
  }
  for (uint32_t f = lane; f < co.n_obs; f += 64) {
    const Obs po = sob[f];
    const uint64_t o = obase + f;
    obs_view[o] = po.view;
    obs_pl[o] = po.pl;
    obs_seg[o] = po.seg;
    *(f2*)(obs_xy + 2 * o) = f2{po.x, po.y};
  }
}

void launch_k4(hipStream_t st, const TaskDesc* tasks, const ChainSeed* chains, uint32_t n_chains, StageBuf stage,
               const ChainOut* outs, const uint32_t* point_off, const uint32_t* obs_off_in, uint64_t point_base,
               uint64_t obs_base, uint32_t key0_base, float* X, eg3d_off_t* obs_off, int32_t* obs_view, uint32_t* obs_pl,
               uint32_t* obs_seg, float* obs_xy, uint32_t* key) {
  if (!n_chains) return;
  hipLaunchKernelGGL(k4_emit, dim3(n_chains), dim3(64), 0, st, tasks, chains, n_chains, stage, outs, point_off,
                     obs_off_in, point_base, obs_base, key0_base, X, obs_off, obs_view, obs_pl, obs_seg, obs_xy, key);
}

}  // namespace eg3d
