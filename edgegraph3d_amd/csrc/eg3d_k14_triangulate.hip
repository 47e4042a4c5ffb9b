// eg3d_k14_triangulate.hip — K14: FP64 triangulation of caller-supplied tracks (include/eg3d_triangulate.h).
//
// compute_3d_point_coords / em_estimate3Dpositions (utils/geometry/triangulation.cpp:178-323, 468-481) and the solve of
// em_add_new_observation_to_3Dpositions (:347-466) on one observation list per track, built from the device statements
// the match kernels use, so that the library has exactly one arithmetic:
//   k14_check   1 lane / track        offsets ascend within [0, n_obs], no list longer than the request table's row count
//   k14_cut     1 lane                the batches: runs of whole tracks whose records fit the staging budget (bisection)
//   k14_stage   1 lane / observation  the caller's SoA rows as the 16-byte Obs records the solver reads; view ids checked
//   k14_solve   1 wave / 32 tracks    [the 2-view DLT on groups of 8 lanes, dlt2_grp8] + coop_gn_groups with the
//                                     long-request path, as k3b_expand calls them; results at the track's own index
// The one-lane form (LocalCursor / triangulate_array for tracks of <= EG3D_LOCAL_OBS rows) is not built.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_pipeline.h"
#include "eg3d_dev_coopgn.h"
#include "eg3d_k14_triangulate.h"

namespace eg3d {

static_assert(K14_MAX_ROWS == 0x7fffu, "a track's row count must fit CoopLds::n16 beside the has-extra bit");
static_assert(sizeof(Obs) == K14_REC_BYTES, "the host sizes the staging area in records of K14_REC_BYTES");
static_assert(EG3D_COOP_REQ == 32, "k14_solve returns the DLT of request 8 r + g from group g of round r: 4 rounds x 8 groups");
static_assert(EG3D_VIEW_BITS + 15 <= 32, "the key of the minimal-view search is view << 15 | row");

// end of track i's list (no sentinel)
__device__ __forceinline__ uint64_t k14_end(const K14Tracks& t, uint64_t i) { return i + 1 < t.n_tracks ? t.obs_off[i + 1] : t.n_obs; }

__global__ void __launch_bounds__(K14_BLOCK) k14_check(K14Tracks t, uint32_t* flags) {
  const uint64_t i = (uint64_t)blockIdx.x * K14_BLOCK + threadIdx.x;
  if (i >= t.n_tracks) return;
  const uint64_t a = t.obs_off[i], b = k14_end(t, i);
  if (!(a <= b && b <= t.n_obs))
    atomicOr(flags, K14_BAD_OFFSETS);
  else if (b - a > (uint64_t)K14_MAX_ROWS)
    atomicOr(flags, K14_LONG_LIST);
}

__global__ void __launch_bounds__(64) k14_cut(K14Tracks t, uint64_t budget, uint64_t cap, unsigned long long* cuts) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  auto off_at = [&](uint64_t i) -> uint64_t { return i < t.n_tracks ? t.obs_off[i] : t.n_obs; };  // i in [0, n_tracks]
  uint64_t nb = 0, t0 = 0;
  while (t0 < t.n_tracks) {
    if (nb == cap) {
      cuts[0] = cap + 1;
      return;
    }
    const uint64_t o0 = off_at(t0);
    cuts[1 + 2 * nb] = t0;
    cuts[2 + 2 * nb] = o0;
    nb++;
    // the largest t1 in (t0, n_tracks] with off_at(t1) - o0 <= budget; t0 + 1 when there is none
    uint64_t lo = t0 + 1, hi = t.n_tracks;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo + 1) / 2;
      const uint64_t om = off_at(mid);
      if (om >= o0 && om - o0 <= budget)
        lo = mid;
      else
        hi = mid - 1;
    }
    t0 = lo;
  }
  cuts[1 + 2 * nb] = t.n_tracks;
  cuts[2 + 2 * nb] = t.n_obs;
  cuts[0] = nb;
}

__global__ void __launch_bounds__(K14_BLOCK) k14_stage(K14Tracks t, int n_views, uint64_t o0, uint64_t o1, Obs* rec, uint32_t* flags) {
  const uint64_t q = o0 + (uint64_t)blockIdx.x * K14_BLOCK + threadIdx.x;
  if (q >= o1) return;
  const int32_t v = t.obs_view[q];
  const bool bad = (uint32_t)v >= (uint32_t)n_views;
  if (bad) atomicOr(flags, K14_BAD_VIEW);
  Obs o;
  o.view = bad ? 0u : (uint32_t)v;
  o.pl = 0;
  o.seg = 0;
  o.x = t.obs_xy[2 * q];
  o.y = t.obs_xy[2 * q + 1];
  rec[q - o0] = o;
}

__global__ void __launch_bounds__(64) k14_solve(const float* cam_P, int cams_mid_range, int mode, K14Tracks t, uint64_t t0, uint64_t t1,
                                                uint64_t o0, const Obs* rec, float* X_out, uint8_t* valid, uint8_t* flags_out,
                                                unsigned long long* counts) {
  __shared__ CoopLds L;
  const int lane = (int)threadIdx.x;
  if (lane == 0) {
    L.cams_mid_range = cams_mid_range ? 1 : 0;
    L.long_refused = 0;
  }
  __syncthreads();
  const uint64_t i = t0 + (uint64_t)blockIdx.x * EG3D_COOP_REQ + (uint64_t)lane;
  const bool mine = lane < EG3D_COOP_REQ && i < t1;
  int n = 0;
  const Obs* base = rec;
  float X0[3] = {0.f, 0.f, 0.f};
  if (mine) {
    const uint64_t a = t.obs_off[i], b = k14_end(t, i);  // (checked: o0 <= a <= b, b - a <= K14_MAX_ROWS, b inside the batch)
    n = (int)(b - a);
    base = rec + (a - o0);
    if (mode == 1) {
      X0[0] = t.X0[3 * i];
      X0[1] = t.X0[3 * i + 1];
      X0[2] = t.X0[3 * i + 2];
    }
  }
  const bool want = mine && n >= 2;
  uint32_t fl = (mine && n < 2) ? K14_OUT_SHORT : 0u;
  const float keep0 = X0[0], keep1 = X0[1], keep2 = X0[2];  // what a track that is not valid gets (+0.0 in mode 0)
  if (mode == 0) {
    // ---- the DLT's entries: the FIRST entry with the minimal view id, and the last entry (triangulate_array)
    int mi = 0;
    if (want && n <= 64) {
      int mv = (int)base[0].view;
      for (int k = 1; k < n; k++) {
        const int v = (int)base[k].view;
        if (v < mv) {
          mv = v;
          mi = k;
        }
      }
    }
    // longer lists one after the other, by the whole wave: the minimum of view << 15 | row names the first minimal entry
    unsigned long long longer = __ballot(want && n > 64);
    while (longer) {
      const int j = __ffsll((long long)longer) - 1;
      longer &= longer - 1ull;
      const int nj = lane_bcast(n, j);
      const Obs* bj = (const Obs*)lane_bcast((unsigned long long)base, j);
      uint32_t best = 0xffffffffu;
      for (int k = lane; k < nj; k += 64) {
        const uint32_t key = ((uint32_t)bj[k].view << 15) | (uint32_t)k;
        best = key < best ? key : best;
      }
      best = wave_min_u32_dpp(best);
      if (lane == j) mi = (int)(best & 0x7fffu);
    }
    int32_t v1 = 0, v2 = 0;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    if (want) {
      const Obs f = base[mi], l = base[n - 1];
      v1 = (int32_t)f.view;
      x1 = f.x;
      y1 = f.y;
      v2 = (int32_t)l.view;
      x2 = l.x;
      y2 = l.y;
      if (v1 == v2) fl |= K14_OUT_DEGENERATE;
    }
    // ---- 32 requests = 4 rounds of 8 lane groups: group g of round r computes the DLT of request 8 r + g
    const int g = lane >> 3;
    for (int r = 0; r < 4; r++) {
      const int src = 8 * r + g;
      const bool on = __shfl(want ? 1 : 0, src) != 0;
      if (!__any(on)) continue;  // wave-uniform
      const int32_t gv1 = __shfl(v1, src), gv2 = __shfl(v2, src);
      const float gx1 = __shfl(x1, src), gy1 = __shfl(y1, src), gx2 = __shfl(x2, src), gy2 = __shfl(y2, src);
      double Xd[3] = {0, 0, 0};
      dlt2_grp8(L.dltg, on, cam_P + (size_t)gv1 * 16, gx1, gy1, cam_P + (size_t)gv2 * 16, gx2, gy2, Xd);
      // (the start point is a float widened to double: it goes back to its request without loss)
      const int from = (lane & 7) * 8;
      const float s0 = __shfl((float)Xd[0], from), s1 = __shfl((float)Xd[1], from), s2 = __shfl((float)Xd[2], from);
      if (g == r) {
        X0[0] = s0;
        X0[1] = s1;
        X0[2] = s2;
      }
    }
  }
  float Xs[3] = {0.f, 0.f, 0.f};
  const bool ok = coop_gn_groups<0, true, EG3D_GN_PRECHECK_IT>(cam_P, L, want, base, n, false, 0, 0.f, 0.f, X0, Xs);
  if (mine) {
    X_out[3 * i] = ok ? Xs[0] : keep0;
    X_out[3 * i + 1] = ok ? Xs[1] : keep1;
    X_out[3 * i + 2] = ok ? Xs[2] : keep2;
    valid[i] = ok ? 1 : 0;
    if (flags_out) flags_out[i] = (uint8_t)fl;
  }
  const int n_ok = __popcll(__ballot(ok)), n_short = __popcll(__ballot((fl & K14_OUT_SHORT) != 0)),
            n_deg = __popcll(__ballot((fl & K14_OUT_DEGENERATE) != 0));
  if (lane == 0) {
    if (n_ok) atomicAdd(&counts[0], (unsigned long long)n_ok);
    if (n_short) atomicAdd(&counts[1], (unsigned long long)n_short);
    if (n_deg) atomicAdd(&counts[2], (unsigned long long)n_deg);
  }
}

void launch_k14_check(hipStream_t st, K14Tracks t, uint32_t* flags) {
  if (!t.n_tracks) return;
  hipLaunchKernelGGL(k14_check, blocks_for(t.n_tracks, K14_BLOCK), dim3(K14_BLOCK), 0, st, t, flags);
}
void launch_k14_cut(hipStream_t st, K14Tracks t, uint64_t budget, uint64_t cap, unsigned long long* cuts) {
  hipLaunchKernelGGL(k14_cut, dim3(1), dim3(64), 0, st, t, budget, cap, cuts);
}
void launch_k14_stage(hipStream_t st, K14Tracks t, int n_views, uint64_t o0, uint64_t o1, Obs* rec, uint32_t* flags) {
  if (o1 <= o0) return;
  hipLaunchKernelGGL(k14_stage, blocks_for(o1 - o0, K14_BLOCK), dim3(K14_BLOCK), 0, st, t, n_views, o0, o1, rec, flags);
}
void launch_k14_solve(hipStream_t st, const float* cam_P, int cams_mid_range, int mode, K14Tracks t, uint64_t t0, uint64_t t1,
                      uint64_t o0, const Obs* rec, float* X_out, uint8_t* valid, uint8_t* flags_out, unsigned long long* counts) {
  if (t1 <= t0) return;
  hipLaunchKernelGGL(k14_solve, blocks_for(t1 - t0, EG3D_COOP_REQ), dim3(64), 0, st, cam_P, cams_mid_range, mode, t, t0, t1, o0, rec,
                     X_out, valid, flags_out, counts);
}

}  // namespace eg3d
