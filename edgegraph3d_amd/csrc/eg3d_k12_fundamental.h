// Host-visible declarations of K12 (eg3d_k12_fundamental.hip): the fundamental matrices of all ordered view pairs from the
// tracks (row N4) on the device. The arithmetic is eg3d_fund_core.h's; these kernels only decide who computes what.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace eg3d {

#define K12_BLOCK 256
#define K12_WAVE 64
#define K12_NO_KEY (~0ull) /* a track entry whose view id is outside the rig */

// One ordered pair with >= 10 common points. The pairs (i, j) and (j, i), i < j, share one list of correspondences
// (x_i, y_i, x_j, y_j as four floats, ascending point id) at pts[off .. off + n); `swap` says the pair reads it as (j, i).
struct K12Pair {
  unsigned long long off;
  uint32_t i, j, n, swap;
};
struct K12Fit {  // one fit: a sample's, or a pair's refit
  double F[9];
  unsigned long long ok;
};
struct K12Normal {  // the refit of a pair, between the selection and its solve
  double A[81];
  double n1[3], n2[3];  // s, cx, cy
  unsigned long long go;  // 1: at least 8 inliers, A is there to be solved
};
struct K12Sel {  // what the selection leaves for the refit's median test
  double best_med;
  unsigned long long have;
};
enum { K12_C_FAILED = 0, K12_C_DEGENERATE = 1, K12_C_EXACT = 2, K12_C_VALID = 3, K12_N_CTR = 4 };

// ---- lists
// key[k] = view << 32 | point of track entry k (K12_NO_KEY outside the rig), val[k] = k; one lane per point
void launch_k12_keys(hipStream_t st, uint32_t n_points, uint32_t n_entries, int32_t n_views, const uint32_t* trk_off, const int32_t* trk_view,
                     unsigned long long* key, uint32_t* val);
// over the stably sorted keys: flag[s] = 1 on the LAST entry of every run of a valid key; flag[n_entries] = 0
void launch_k12_heads(hipStream_t st, uint32_t n_entries, const unsigned long long* skey, uint32_t* flag);
// the observations: ckey[pos[s]] = skey[s], cxy[pos[s]] = trk_xy[sval[s]] where flag[s]
void launch_k12_compact(hipStream_t st, uint32_t n_entries, const unsigned long long* skey, const uint32_t* sval, const uint32_t* flag,
                        const uint32_t* pos, const float* trk_xy, unsigned long long* ckey, float2* cxy);
// voff[v] = the first observation of view v, v <= n_views
void launch_k12_view_off(hipStream_t st, int32_t n_views, uint32_t n_obs, const unsigned long long* ckey, uint32_t* voff);
// one wavefront per unordered pair i < j (a grid over all V * V slots u = i * V + j): the shorter list searched in the longer.
//   fill = false: ncom[i][j] = ncom[j][i] = the count; has[u] = count >= 10; size[u] = has ? count : 0 (0 in every other slot)
//   fill = true:  the correspondences of slot u placed by rank at pts[size_off[u] ..), and the two pair records at
//                 pairs[2 * has_rank[u]], [2 * has_rank[u] + 1]
void launch_k12_common(hipStream_t st, bool fill, int32_t n_views, const uint32_t* voff, const unsigned long long* ckey, const float2* cxy,
                       uint32_t* ncom, uint32_t* has, unsigned long long* size, const uint32_t* has_rank, const unsigned long long* size_off,
                       float4* pts, K12Pair* pairs);
// ---- per chunk of pairs [p0, p0 + n_pairs)
// one lane per pair walks its stream: idx[(pair - p0) * iterations + it][8]
void launch_k12_samples(hipStream_t st, uint32_t p0, uint32_t n_pairs, uint32_t iterations, int32_t n_views, unsigned long long rng_seed,
                        const K12Pair* pairs, uint32_t* idx);
// the hot kernel, one lane per fit. normals == nullptr: fit (pair - p0) * iterations + it from its sample; otherwise fit
// (pair - p0) from the pair's normal matrix (the refit)
void launch_k12_fit(hipStream_t st, uint32_t p0, uint32_t n_pairs, uint32_t iterations, const K12Pair* pairs, const float4* pts,
                    const uint32_t* idx, const K12Normal* normals, K12Fit* fits);
// one wavefront per pair: the walk over its fits, the exact medians it needs, the inliers, the refit's normal matrix.
// F / F_valid receive the best sample's matrix. err / inl: 2 * (all correspondences) words of scratch each.
void launch_k12_select(hipStream_t st, uint32_t p0, uint32_t n_pairs, uint32_t iterations, uint32_t stage_points, int32_t n_views,
                       const K12Pair* pairs, const float4* pts, const K12Fit* fits, unsigned long long* err, uint32_t* inl,
                       K12Normal* normals, K12Sel* sel, double* F, uint8_t* F_valid, unsigned long long* ctr);
// one wavefront per pair: the refit replaces the matrix if its median is <= the best
void launch_k12_final(hipStream_t st, uint32_t p0, uint32_t n_pairs, int32_t n_views, const K12Pair* pairs, const float4* pts,
                      const K12Fit* refits, const K12Sel* sel, double* F);

}  // namespace eg3d
