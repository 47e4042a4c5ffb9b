// eg3d_k5_filter.hip — K5 (gfx950):
//   k5_gn_filter      1 lane / point        config 5, FP32 Gauss-Newton outlier filter
// All arithmetic follows the contract in DESIGN.md (no FMA contraction: -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_pipeline.h"
#include "eg3d_kernels.h"

namespace eg3d {

// ------------------------------------------------------------------ K5 ---------
// One lane per point, one block per 256 consecutive points. The block's operands are staged in LDS
// with coalesced loads first: the 3x4 part of every camera matrix (V <= 256) and the block's
// observations, which are one contiguous slice of the CSR (<= K5_OBS_CAP of them; k ~ U[3,10] gives
// ~1.5k). A lane then walks ITS list through ds_reads — lane-strided reads of the CSR straight from
// HBM touch ~7x the cache lines they use, and the per-observation camera matrix is a 48-byte gather.
// Blocks whose slice or rig does not fit fall back to the HBM operands (same arithmetic).
// What bounds it is arithmetic, not memory: the filter's convergence test |d mse| < 5e-10 on FP32 values
// of ~0.25 only fires when the mean-square error repeats EXACTLY, so most points run many of the 30
// iterations, each 2 passes x k rows x (8 correctly rounded FP32 divisions + 60 FP64 multiply-adds and
// conversions). Measured alternatives (same bits, slower): persistent lanes with a flattened
// per-row state machine and a global work counter — the end-of-pass step then diverges on almost every
// trip (4.4 ms vs 3.2 ms per 1 M points).
// Round 6 — lane occupancy (tools/c5_iterations.py: on the 1 M-point workload 62 % of the points run all 30 passes, the
// others stop after 4-10, and k spans 3..10; with points taken in input order a wavefront keeps 0.71 of its lanes busy by
// passes and only 0.41 by residual rows, because every pass runs as long as the longest list among its 64 lanes). The
// block's points are therefore SORTED BY k in LDS (counting sort) before lanes take them: a wavefront's lists have (nearly)
// the same length. 2.83 -> 2.17 ms per 1 M points, vector instructions 1.78e9 -> 1.18e9, measured active-lane fraction
// 0.61 (profiles/r06_c5_rocprof_summary.txt). A point's arithmetic does not depend on the lane that runs it, so the output
// is bit for bit what one lane per point in input order produces.
// Measured and dropped: packing the points still running after 6 / 10 passes into the block's first wavefronts (state
// through LDS, order kept; gauss_newton_f32_span makes the iteration resumable): 2.37 / 2.21 ms against 2.17 without —
// a block of 4 wavefronts rarely empties a whole one (0.62 x 256 points = 2.5 wavefronts), and the freed lanes of a
// partly empty wavefront cost nothing extra.
#define K5_BLOCK 256
#define K5_OBS_CAP 2816
#define K5_VIEW_CAP 256
#define K5_KBUCKETS 65 /* list lengths 0..63 and "64 or more" */
// The body has two instantiations. <uint32_t, true>: host clouds as eg3d_gn_filter uploads them (32-bit offsets with a
// sentinel, validated on the host; ext is empty). <uint64_t, false>: device-resident clouds as the match path leaves them
// (eg3d_device_edgepoints: 64-bit offsets, the last point ends at ext.n_obs), which nothing has validated: a list that
// does not lie inside [0, n_obs] in ascending order, or a view id outside the rig, raises a bit of *ext.flags and the
// point is skipped (no operand is read through a bad index). This form also takes the optional keep mask (a masked
// point takes bucket 0 of the counting sort and costs no arithmetic) and accumulates the histogram of the inliers' list
// lengths where the verdict and k are in registers: LDS bins per block and one 64-bit atomic per non-empty bin for rigs
// of <= K5_VIEW_CAP views, global atomics otherwise (block-uniform). ext.hist has n_views + 2 bins: [k] for k <= n_views,
// [n_views + 1] for longer lists.
#define K5_SKIP 0x8000u /* s_perm: the point is masked out or malformed */
template <typename OffT, bool SENTINEL>
__global__ void __launch_bounds__(K5_BLOCK) k5_gn_filter(const float* cam_P, int n_views, const float* X,
                                                        const OffT* obs_off, const int32_t* obs_view,
                                                        const float* obs_xy, uint64_t n, float gn_max_mse,
                                                        int legacy_abs, float* X_out, uint8_t* inlier,
                                                        K5Ext<SENTINEL> ext) {
  typedef const __attribute__((address_space(3))) float* lds_fp;
  typedef const __attribute__((address_space(3))) int32_t* lds_ip;
  __shared__ float sP[K5_VIEW_CAP * 12];
  __shared__ int32_t sV[K5_OBS_CAP];
  __shared__ float sXY[2 * K5_OBS_CAP];
  __shared__ uint32_t s_cnt[K5_KBUCKETS], s_base[K5_KBUCKETS];
  __shared__ uint16_t s_perm[K5_BLOCK];
  __shared__ uint32_t s_hist[SENTINEL ? 1 : K5_VIEW_CAP + 2];  // (never referenced by the host-cloud form: no LDS there)
  const uint64_t p0 = (uint64_t)blockIdx.x * K5_BLOCK;
  const uint64_t p1 = p0 + K5_BLOCK < n ? p0 + K5_BLOCK : n;
  const uint32_t np = (uint32_t)(p1 - p0);
  // end of point i's list
  auto off_end = [&](uint64_t i) -> OffT {
    if constexpr (SENTINEL)
      return obs_off[i + 1];
    else
      return i + 1 < n ? obs_off[i + 1] : (OffT)ext.n_obs;
  };
  const OffT o0 = obs_off[p0], o1 = off_end(p1 - 1);
  // the block's slice: a 64-bit difference on device clouds, held in 32 bits once it is known to fit the staging area
  bool fits;
  if constexpr (SENTINEL)
    fits = (uint32_t)(o1 - o0) <= K5_OBS_CAP;
  else
    fits = o0 <= o1 && o1 <= ext.n_obs && o1 - o0 <= (OffT)K5_OBS_CAP;
  const uint32_t m = (uint32_t)(o1 - o0);
  const uint32_t t = threadIdx.x;
  const bool staged = n_views <= K5_VIEW_CAP && fits;  // block-uniform
  if (staged) {
    for (uint32_t q = t; q < (uint32_t)n_views * 12u; q += K5_BLOCK) sP[q] = cam_P[(q / 12u) * 16u + q % 12u];
    if constexpr (SENTINEL) {
      for (uint32_t q = t; q < m; q += K5_BLOCK) sV[q] = obs_view[o0 + q];
    } else {
      bool bad_view = false;
      for (uint32_t q = t; q < m; q += K5_BLOCK) {
        const int32_t v = obs_view[o0 + q];
        const bool bad = (uint32_t)v >= (uint32_t)n_views;
        bad_view |= bad;
        sV[q] = bad ? 0 : v;
      }
      if (bad_view) atomicOr(ext.flags, K5_FLAG_BAD_VIEW);
    }
    for (uint32_t q = t; q < 2u * m; q += K5_BLOCK) sXY[q] = obs_xy[2 * (size_t)o0 + q];
  }
  if (t < K5_KBUCKETS) s_cnt[t] = 0;
  if constexpr (!SENTINEL) {
    if (n_views <= K5_VIEW_CAP)
      for (uint32_t q = t; q < (uint32_t)n_views + 2u; q += K5_BLOCK) s_hist[q] = 0;
  }
  __syncthreads();
  // ---- (1) counting sort of the block's points by list length (the order inside a bucket is whatever the LDS atomics
  // give: it decides which lane runs a point, not what the point computes)
  uint32_t kb = 0, rank = 0;
  bool skip = false;
  if (t < np) {
    if constexpr (SENTINEL) {
      const uint32_t k = obs_off[p0 + t + 1] - obs_off[p0 + t];
      kb = k < K5_KBUCKETS - 1 ? k : K5_KBUCKETS - 1;
    } else {
      const OffT a = obs_off[p0 + t], b = off_end(p0 + t);
      bool bad = !(a <= b && b <= ext.n_obs && b - a <= (OffT)K5_MAX_LIST) || (staged && !(a >= o0 && b <= o1));
      if (!bad && !staged) {  // operands come straight from HBM: no view id may index past the rig's cameras
        bool bad_view = false;
        for (OffT q = a; q < b; q++) bad_view |= (uint32_t)obs_view[q] >= (uint32_t)n_views;
        if (bad_view) atomicOr(ext.flags, K5_FLAG_BAD_VIEW);
        bad = bad_view;
      } else if (bad) {
        atomicOr(ext.flags, K5_FLAG_BAD_OFFSETS);
      }
      skip = bad || (ext.keep && !ext.keep[p0 + t]);
      const OffT k = skip ? 0 : b - a;
      kb = k < K5_KBUCKETS - 1 ? (uint32_t)k : K5_KBUCKETS - 1;
    }
    rank = atomicAdd(&s_cnt[kb], 1u);
  }
  __syncthreads();
  if (t < K5_KBUCKETS) {
    uint32_t base = 0;
    for (uint32_t q = 0; q < t; q++) base += s_cnt[q];
    s_base[t] = base;
  }
  __syncthreads();
  if constexpr (SENTINEL) {
    if (t < np) s_perm[s_base[kb] + rank] = (uint16_t)t;
  } else {
    if (t < np) s_perm[s_base[kb] + rank] = (uint16_t)(t | (skip ? K5_SKIP : 0u));
  }
  __syncthreads();
  // ---- lane t takes the t-th point of the sorted order
  auto run_span = [&](uint32_t j, GnF32State& st, int it0, int it1) -> int {
    const uint64_t i = p0 + j;
    const OffT a = obs_off[i], b = off_end(i);
    if (staged)
      return gauss_newton_f32_span((lds_fp)&sP[0], 12, (lds_ip)&sV[0] + (a - o0), (lds_fp)&sXY[0] + 2 * (a - o0), (int)(b - a),
                                   st, legacy_abs != 0, it0, it1);
    return gauss_newton_f32_span(cam_P, 16, obs_view + a, obs_xy + 2 * (size_t)a, (int)(b - a), st, legacy_abs != 0, it0, it1);
  };
  auto finish = [&](uint32_t j, const GnF32State& st, int r) -> bool {  // gauss_newton.cpp:130-133: accepted on the last mse, converged or not
    const uint64_t i = p0 + j;
    const bool ok = r != GN_F32_FAILED && st.last_mse < gn_max_mse;
    const float x0 = X[3 * i], x1 = X[3 * i + 1], x2 = X[3 * i + 2];
    inlier[i] = ok ? 1 : 0;
    X_out[3 * i] = ok ? st.X[0] : x0;
    X_out[3 * i + 1] = ok ? st.X[1] : x1;
    X_out[3 * i + 2] = ok ? st.X[2] : x2;
    return ok;
  };
  if constexpr (SENTINEL) {
    if (t < np) {
      const uint32_t j = s_perm[t];
      const uint64_t i = p0 + j;
      GnF32State st;
      st.X[0] = X[3 * i];
      st.X[1] = X[3 * i + 1];
      st.X[2] = X[3 * i + 2];
      st.last_mse = 0;
      finish(j, st, run_span(j, st, 0, 30));
    }
  } else {
    const bool lds_bins = n_views <= K5_VIEW_CAP;  // block-uniform
    if (t < np) {
      const uint32_t pj = s_perm[t];
      const uint32_t j = pj & (K5_SKIP - 1u);
      const uint64_t i = p0 + j;
      GnF32State st;
      st.X[0] = X[3 * i];
      st.X[1] = X[3 * i + 1];
      st.X[2] = X[3 * i + 2];
      st.last_mse = 0;
      if (pj & K5_SKIP) {
        inlier[i] = 0;
        X_out[3 * i] = st.X[0];
        X_out[3 * i + 1] = st.X[1];
        X_out[3 * i + 2] = st.X[2];
      } else if (finish(j, st, run_span(j, st, 0, 30))) {
        const OffT k = off_end(i) - obs_off[i];
        const uint32_t bin = k <= (OffT)n_views ? (uint32_t)k : (uint32_t)n_views + 1u;
        if (lds_bins)
          atomicAdd(&s_hist[bin], 1u);
        else
          atomicAdd(ext.hist + bin, 1ull);
      }
    }
    if (lds_bins) {
      __syncthreads();
      for (uint32_t q = t; q < (uint32_t)n_views + 2u; q += K5_BLOCK) {
        const uint32_t c = s_hist[q];
        if (c) atomicAdd(ext.hist + q, (unsigned long long)c);
      }
    }
  }
}

void launch_k5(hipStream_t st, const float* cam_P, int n_views, const float* X, const uint32_t* obs_off,
               const int32_t* obs_view, const float* obs_xy, uint64_t n, float gn_max_mse, int legacy_abs, float* X_out,
               uint8_t* inlier) {
  if (!n) return;
  hipLaunchKernelGGL((k5_gn_filter<uint32_t, true>), blocks_for(n, K5_BLOCK), dim3(K5_BLOCK), 0, st, cam_P, n_views, X, obs_off,
                     obs_view, obs_xy, n, gn_max_mse, legacy_abs, X_out, inlier, K5Host{});
}
void launch_k5_device(hipStream_t st, const float* cam_P, int n_views, const float* X, const eg3d_off_t* obs_off,
                      const int32_t* obs_view, const float* obs_xy, uint64_t n, float gn_max_mse, int legacy_abs, float* X_out,
                      uint8_t* inlier, K5Dev ext) {
  if (!n) return;
  hipLaunchKernelGGL((k5_gn_filter<eg3d_off_t, false>), blocks_for(n, K5_BLOCK), dim3(K5_BLOCK), 0, st, cam_P, n_views, X,
                     obs_off, obs_view, obs_xy, n, gn_max_mse, legacy_abs, X_out, inlier, ext);
}

}  // namespace eg3d
