// eg3d_k12_fundamental.hip — K12: the fundamental matrices of all ordered view pairs from the tracks (row N4,
// eg3d_estimate_fundamental). Every number is computed by the functions of eg3d_fund_core.h, which the host statement
// (host/fundamental.cpp) uses in the plain way; the kernels only distribute the work, and every place is given by a rank
// (a scan, a ballot), never by the order in which lanes arrive. Sums whose order is part of the arithmetic are made by
// ONE lane each, in that order.
//   k12_keys / heads / compact / view_off   1 lane / point, sorted entry, view      the observations, sorted by (view, point)
//   k12_common<fill>                        1 WAVE / unordered pair                 counts; then the correspondences by rank
//   k12_samples                             1 lane / pair                           the pair's SplitMix64 stream
//   k12_fit                                 1 lane / fit, 1 wave / SIMD             normal matrix + both Jacobis in registers
//   k12_select                              1 WAVE / pair                           walk, exact medians, inliers, refit's A
//   k12_final                               1 WAVE / pair                           the refit's median test
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_fund_core.h"
#include "eg3d_k12_fundamental.h"

namespace eg3d {

typedef unsigned long long u64;
using fund::Corr;

__device__ __forceinline__ uint32_t k12_wave_sum(uint32_t v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// what the lanes of this wavefront wrote to memory is there for its other lanes
__device__ __forceinline__ void k12_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ u64 k12_bits(double x) { return (u64)__double_as_longlong(x); }

// ---- lists ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(K12_BLOCK) k12_keys(uint32_t n_points, uint32_t n_entries, int32_t n_views, const uint32_t* trk_off,
                                                      const int32_t* trk_view, u64* key, uint32_t* val) {
  const u64 p = (u64)blockIdx.x * K12_BLOCK + threadIdx.x;
  if (p >= n_points) return;
  const uint32_t b = trk_off[p], e = min(trk_off[p + 1], n_entries);  // (the driver has checked the offsets; the bound stays)
  for (uint32_t k = b; k < e; k++) {
    const int32_t v = trk_view[k];
    key[k] = (v < 0 || v >= n_views) ? K12_NO_KEY : ((u64)(uint32_t)v << 32 | p);
    val[k] = k;
  }
}

__global__ void __launch_bounds__(K12_BLOCK) k12_heads(uint32_t n_entries, const u64* skey, uint32_t* flag) {
  const u64 s = (u64)blockIdx.x * K12_BLOCK + threadIdx.x;
  if (s > n_entries) return;
  uint32_t f = 0;
  if (s < n_entries) {
    const u64 k = skey[s];
    f = k != K12_NO_KEY && (s + 1 == n_entries || skey[s + 1] != k);
  }
  flag[s] = f;
}

__global__ void __launch_bounds__(K12_BLOCK) k12_compact(uint32_t n_entries, const u64* skey, const uint32_t* sval, const uint32_t* flag,
                                                         const uint32_t* pos, const float* trk_xy, u64* ckey, float2* cxy) {
  const u64 s = (u64)blockIdx.x * K12_BLOCK + threadIdx.x;
  if (s >= n_entries || !flag[s]) return;
  const uint32_t c = pos[s], k = sval[s];
  ckey[c] = skey[s];
  cxy[c] = make_float2(trk_xy[2 * (size_t)k], trk_xy[2 * (size_t)k + 1]);
}

// first c in [lo, hi) with ckey[c] >= want
__device__ __forceinline__ uint32_t k12_lower_bound(const u64* ckey, uint32_t lo, uint32_t hi, u64 want) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ckey[mid] < want) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(K12_BLOCK) k12_view_off(int32_t n_views, uint32_t n_obs, const u64* ckey, uint32_t* voff) {
  const uint32_t v = blockIdx.x * K12_BLOCK + threadIdx.x;
  if (v > (uint32_t)n_views) return;
  voff[v] = k12_lower_bound(ckey, 0, n_obs, (u64)v << 32);
}

template <bool FILL>
__global__ void __launch_bounds__(K12_WAVE) k12_common(int32_t n_views, const uint32_t* voff, const u64* ckey, const float2* cxy,
                                                       uint32_t* ncom, uint32_t* has, u64* size, const uint32_t* has_rank,
                                                       const u64* size_off, float4* pts, K12Pair* pairs) {
  const uint32_t V = (uint32_t)n_views;
  const uint32_t u = blockIdx.x, i = u / V, j = u % V, lane = threadIdx.x;
  if (i >= j) {
    if (!FILL && lane == 0) {
      has[u] = 0;
      size[u] = 0;
      if (i == j) ncom[u] = 0;
    }
    return;
  }
  if (FILL && !has[u]) return;
  const uint32_t bi = voff[i], ei = voff[i + 1], bj = voff[j], ej = voff[j + 1];
  const bool i_short = ei - bi <= ej - bj;
  const uint32_t sb = i_short ? bi : bj, se = i_short ? ei : ej, lb = i_short ? bj : bi, le = i_short ? ej : ei;
  const u64 lview = (u64)(i_short ? j : i) << 32;
  const u64 out = FILL ? size_off[u] : 0;
  uint32_t count = 0;
  for (uint32_t base = sb; base < se; base += K12_WAVE) {  // (wave-uniform bounds)
    const uint32_t k = base + lane;
    bool found = false;
    uint32_t at = 0;
    if (k < se) {
      const u64 want = lview | (ckey[k] & 0xFFFFFFFFull);
      at = k12_lower_bound(ckey, lb, le, want);
      found = at < le && ckey[at] == want;
    }
    const u64 m = __ballot(found);
    if (FILL && found) {
      const uint32_t r = count + __popcll(m & ((1ull << lane) - 1));  // ascending point id: the short list is ascending
      const float2 a = cxy[i_short ? k : at], b = cxy[i_short ? at : k];  // a: on view i, b: on view j
      pts[out + r] = make_float4(a.x, a.y, b.x, b.y);
    }
    count += (uint32_t)__popcll(m);
  }
  if (lane) return;
  if (!FILL) {
    ncom[(size_t)i * V + j] = ncom[(size_t)j * V + i] = count;
    has[u] = count >= (uint32_t)fund::kMinCommon;
    size[u] = count >= (uint32_t)fund::kMinCommon ? count : 0;
  } else {
    const uint32_t r = has_rank[u];
    pairs[2 * (size_t)r] = K12Pair{out, i, j, count, 0};
    pairs[2 * (size_t)r + 1] = K12Pair{out, j, i, count, 1};
  }
}

// ---- samples ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(K12_BLOCK) k12_samples(uint32_t p0, uint32_t n_pairs, uint32_t iterations, int32_t n_views, u64 rng_seed,
                                                         const K12Pair* pairs, uint32_t* idx) {
  const uint32_t pl = blockIdx.x * K12_BLOCK + threadIdx.x;
  if (pl >= n_pairs) return;
  const K12Pair pr = pairs[p0 + pl];
  fund::Rng rng{fund::stream_seed(rng_seed, (u64)pr.i * (uint32_t)n_views + pr.j)};
  uint4* out = reinterpret_cast<uint4*>(idx + (size_t)pl * iterations * 8);
  for (uint32_t it = 0; it < iterations; it++) {
    uint32_t s[fund::kSample];
    fund::draw_sample(rng, pr.n, s);
    out[2 * (size_t)it] = make_uint4(s[0], s[1], s[2], s[3]);
    out[2 * (size_t)it + 1] = make_uint4(s[4], s[5], s[6], s[7]);
  }
}

// ---- fits -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Corr k12_corr(float4 q, uint32_t swap) {
  return swap ? Corr{(double)q.z, (double)q.w, (double)q.x, (double)q.y} : Corr{(double)q.x, (double)q.y, (double)q.z, (double)q.w};
}

// One lane per fit, one wavefront per SIMD: A and V of the 9 x 9 Jacobi are 162 doubles per lane and live in the unified
// VGPR / AGPR file. Lanes leave the sweep loop at different sweeps; the wavefront runs until its slowest lane is done.
__global__ void __launch_bounds__(K12_WAVE) k12_fit(uint32_t p0, uint32_t n_pairs, uint32_t iterations, const K12Pair* pairs,
                                                    const float4* pts, const uint32_t* idx, const K12Normal* normals, K12Fit* fits) {
  const u64 g = (u64)blockIdx.x * K12_WAVE + threadIdx.x;
  double A[9][9], F[9];
  fund::Norm n1, n2;
  if (normals == nullptr) {
    if (g >= (u64)n_pairs * iterations) return;
    const K12Pair pr = pairs[p0 + (uint32_t)(g / iterations)];
    const uint32_t* ix = idx + g * 8;
    const float4* pp = pts + pr.off;
    fund::build_normal([&](int k) { return k12_corr(pp[ix[k]], pr.swap); }, fund::kSample, n1, n2, A);
  } else {
    if (g >= n_pairs) return;
    const K12Normal* nm = normals + g;
    if (!nm->go) {
      fits[g].ok = 0;
      return;
    }
    EG3D_FUND_UNROLL
    for (int a = 0; a < 9; a++) {
      EG3D_FUND_UNROLL
      for (int b = 0; b < 9; b++) A[a][b] = nm->A[9 * a + b];
    }
    n1 = fund::Norm{nm->n1[0], nm->n1[1], nm->n1[2]};
    n2 = fund::Norm{nm->n2[0], nm->n2[1], nm->n2[2]};
  }
  const bool ok = fund::solve_normal(A, n1, n2, F);
  K12Fit* f = fits + g;
  EG3D_FUND_UNROLL
  for (int a = 0; a < 9; a++) f->F[a] = F[a];
  f->ok = ok ? 1ull : 0ull;
}

// ---- selection --------------------------------------------------------------------------------------------------------------
// a pair's correspondences as the selection reads them: staged in LDS in the pair's own orientation, or from memory
struct K12Points {
  const float4* lds;  // nullptr: the pair is longer than the staging area
  const float4* mem;
  uint32_t swap;
  __device__ __forceinline__ Corr operator()(uint32_t k) const { return lds ? k12_corr(lds[k], 0) : k12_corr(mem[k], swap); }
};

// lanes count the correspondences whose residual under F is below (or not above) `bound`
template <bool OR_EQUAL>
__device__ __forceinline__ uint32_t k12_count(const double (&F)[9], const K12Points& P, uint32_t n, uint32_t lane, double bound) {
  uint32_t c = 0;
  for (uint32_t k = lane; k < n; k += K12_WAVE) {
    const double e = fund::residual(F, P(k));
    c += OR_EQUAL ? e <= bound : e < bound;
  }
  return k12_wave_sum(c);
}

// The r-th smallest (from zero) residual under F. Residuals are +0, positive or kHuge: their bit patterns order as unsigned
// integers, and the r-th smallest is the largest x with fewer than r + 1 values below it, found bit by bit. Every lane keeps
// the keys k = lane, lane + 64, .. it computed itself in `key` (memory: no capacity to outgrow).
__device__ __forceinline__ double k12_exact(const double (&F)[9], const K12Points& P, uint32_t n, uint32_t lane, uint32_t r, u64* key) {
  for (uint32_t k = lane; k < n; k += K12_WAVE) key[k] = k12_bits(fund::residual(F, P(k)));
  u64 x = 0;
  for (int bit = 62; bit >= 0; bit--) {  // (bit 63 is the sign: never set)
    const u64 cand = x | (1ull << bit);
    uint32_t c = 0;
    for (uint32_t k = lane; k < n; k += K12_WAVE) c += key[k] < cand;
    if (k12_wave_sum(c) <= r) x = cand;
  }
  return __longlong_as_double((long long)x);
}

extern __shared__ float4 k12_stage[];

__global__ void __launch_bounds__(K12_WAVE) k12_select(uint32_t p0, uint32_t iterations, uint32_t stage_points, int32_t n_views,
                                                       const K12Pair* pairs, const float4* pts, const K12Fit* fits, u64* err,
                                                       uint32_t* inl, K12Normal* normals, K12Sel* sel, double* Fout, uint8_t* F_valid,
                                                       u64* ctr) {
  const uint32_t pl = blockIdx.x, lane = threadIdx.x;
  const K12Pair pr = pairs[p0 + pl];
  const uint32_t n = pr.n;
  const bool staged = n <= stage_points;
  if (staged) {
    for (uint32_t k = lane; k < n; k += K12_WAVE) {
      const float4 q = pts[pr.off + k];
      k12_stage[k] = pr.swap ? make_float4(q.z, q.w, q.x, q.y) : q;
    }
    __syncthreads();
  }
  const K12Points P{staged ? k12_stage : nullptr, pts + pr.off, pr.swap};
  u64* const key = err + 2 * pr.off + (u64)pr.swap * n;
  uint32_t* const in = inl + 2 * pr.off + (u64)pr.swap * n;
  const K12Fit* const pf = fits + (size_t)pl * iterations;
  const uint32_t need = n / 2 + 1;  // the n/2-th smallest is below x exactly when at least n/2 + 1 values are

  double best = fund::kHuge;
  uint32_t best_it = 0xFFFFFFFFu, n_degenerate = 0, n_exact = 0;
  for (uint32_t it = 0; it < iterations; it++) {  // (everything the loop branches on is wave-uniform)
    const K12Fit* f = pf + it;
    if (!f->ok) {
      n_degenerate++;
      continue;
    }
    double F[9];
    EG3D_FUND_UNROLL
    for (int a = 0; a < 9; a++) F[a] = f->F[a];
    if (k12_count<false>(F, P, n, lane, best) < need) continue;  // its median is not below the best
    best = k12_exact(F, P, n, lane, n / 2, key);
    best_it = it;
    n_exact++;
  }
  K12Normal* const nm = normals + pl;
  const size_t ij = (size_t)pr.i * (uint32_t)n_views + pr.j;
  if (lane == 0) {
    if (n_degenerate) atomicAdd(ctr + K12_C_DEGENERATE, (u64)n_degenerate);
    if (n_exact) atomicAdd(ctr + K12_C_EXACT, (u64)n_exact);
    atomicAdd(ctr + (best_it == 0xFFFFFFFFu ? K12_C_FAILED : K12_C_VALID), 1ull);
    sel[pl] = K12Sel{best, best_it != 0xFFFFFFFFu};
    nm->go = 0;
  }
  if (best_it == 0xFFFFFFFFu) return;  // every sample degenerate, or no finite median: no matrix (F and F_valid stay 0)
  double F[9];
  EG3D_FUND_UNROLL
  for (int a = 0; a < 9; a++) F[a] = pf[best_it].F[a];
  if (lane < 9) Fout[ij * 9 + lane] = pf[best_it].F[lane];
  if (lane == 0) F_valid[ij] = 1;

  // the inliers, ascending, placed by ballot rank
  const double thr = fund::inlier_threshold(best, (int)n);
  uint32_t n_in = 0;
  for (uint32_t base = 0; base < n; base += K12_WAVE) {
    const uint32_t k = base + lane;
    const bool is_in = k < n && fund::residual(F, P(k)) <= thr;
    const u64 m = __ballot(is_in);
    if (is_in) in[n_in + __popcll(m & ((1ull << lane) - 1))] = k;
    n_in += (uint32_t)__popcll(m);
  }
  if (n_in < (uint32_t)fund::kSample) return;
  k12_wave_sync();
  // The refit's normalisation and normal matrix, as fund::build_normal over the inliers: every sum by ONE lane in ascending
  // order. Lanes 0..3 the centroid sums, lanes 0..1 the distance sums, then one lane per entry of A (81 entries on 64
  // lanes: lanes 0..16 carry a second one). The other lanes run along on copies.
  const double dn = (double)(int)n_in;
  double s = 0;
  for (uint32_t m = 0; m < n_in; m++) {
    const Corr p = P(in[m]);
    const uint32_t w = lane & 3;
    s += w == 0 ? p.x1 : w == 1 ? p.y1 : w == 2 ? p.x2 : p.y2;
  }
  s /= dn;
  const double cx1 = __shfl(s, 0, 64), cy1 = __shfl(s, 1, 64), cx2 = __shfl(s, 2, 64), cy2 = __shfl(s, 3, 64);
  double d = 0;
  for (uint32_t m = 0; m < n_in; m++) {
    const Corr p = P(in[m]);
    d += (lane & 1) ? fund::norm_dist(p.x2 - cx2, p.y2 - cy2) : fund::norm_dist(p.x1 - cx1, p.y1 - cy1);
  }
  d /= dn;
  const double sc = fund::norm_scale(d);
  const double s1 = __shfl(sc, 0, 64), s2 = __shfl(sc, 1, 64);
  const int e0 = (int)lane, e1 = min((int)lane + 64, 80);
  const int a0 = e0 / 9, b0 = e0 % 9, a1 = e1 / 9, b1 = e1 % 9;
  double acc0 = 0, acc1 = 0;
  for (uint32_t m = 0; m < n_in; m++) {
    const Corr p = P(in[m]);
    const double x1 = (p.x1 - cx1) * s1, y1 = (p.y1 - cy1) * s1;
    const double x2 = (p.x2 - cx2) * s2, y2 = (p.y2 - cy2) * s2;
    acc0 += fund::row_entry(a0, x1, y1, x2, y2) * fund::row_entry(b0, x1, y1, x2, y2);
    acc1 += fund::row_entry(a1, x1, y1, x2, y2) * fund::row_entry(b1, x1, y1, x2, y2);
  }
  nm->A[e0] = acc0;
  if (lane + 64 < 81) nm->A[lane + 64] = acc1;
  if (lane == 0) {
    nm->n1[0] = s1;
    nm->n1[1] = cx1;
    nm->n1[2] = cy1;
    nm->n2[0] = s2;
    nm->n2[1] = cx2;
    nm->n2[2] = cy2;
    nm->go = 1;
  }
}

__global__ void __launch_bounds__(K12_WAVE) k12_final(uint32_t p0, int32_t n_views, const K12Pair* pairs, const float4* pts,
                                                      const K12Fit* refits, const K12Sel* sel, double* Fout) {
  const uint32_t pl = blockIdx.x, lane = threadIdx.x;
  if (!sel[pl].have || !refits[pl].ok) return;
  const K12Pair pr = pairs[p0 + pl];
  const K12Points P{nullptr, pts + pr.off, pr.swap};
  double F[9];
  EG3D_FUND_UNROLL
  for (int a = 0; a < 9; a++) F[a] = refits[pl].F[a];
  // kept only if its median is <= the best: at least n/2 + 1 residuals are
  if (k12_count<true>(F, P, pr.n, lane, sel[pl].best_med) < pr.n / 2 + 1) return;
  if (lane < 9) Fout[((size_t)pr.i * (uint32_t)n_views + pr.j) * 9 + lane] = refits[pl].F[lane];
}

// ---- launches ---------------------------------------------------------------------------------------------------------------
static inline uint32_t k12_blocks(u64 n) { return (uint32_t)((n + K12_BLOCK - 1) / K12_BLOCK); }

void launch_k12_keys(hipStream_t st, uint32_t n_points, uint32_t n_entries, int32_t n_views, const uint32_t* trk_off, const int32_t* trk_view,
                     u64* key, uint32_t* val) {
  if (!n_points) return;
  k12_keys<<<k12_blocks(n_points), K12_BLOCK, 0, st>>>(n_points, n_entries, n_views, trk_off, trk_view, key, val);
}
void launch_k12_heads(hipStream_t st, uint32_t n_entries, const u64* skey, uint32_t* flag) {
  k12_heads<<<k12_blocks((u64)n_entries + 1), K12_BLOCK, 0, st>>>(n_entries, skey, flag);
}
void launch_k12_compact(hipStream_t st, uint32_t n_entries, const u64* skey, const uint32_t* sval, const uint32_t* flag, const uint32_t* pos,
                        const float* trk_xy, u64* ckey, float2* cxy) {
  if (!n_entries) return;
  k12_compact<<<k12_blocks(n_entries), K12_BLOCK, 0, st>>>(n_entries, skey, sval, flag, pos, trk_xy, ckey, cxy);
}
void launch_k12_view_off(hipStream_t st, int32_t n_views, uint32_t n_obs, const u64* ckey, uint32_t* voff) {
  k12_view_off<<<k12_blocks((u64)n_views + 1), K12_BLOCK, 0, st>>>(n_views, n_obs, ckey, voff);
}
void launch_k12_common(hipStream_t st, bool fill, int32_t n_views, const uint32_t* voff, const u64* ckey, const float2* cxy, uint32_t* ncom,
                       uint32_t* has, u64* size, const uint32_t* has_rank, const u64* size_off, float4* pts, K12Pair* pairs) {
  const uint32_t slots = (uint32_t)n_views * (uint32_t)n_views;  // (n_views <= 8192: at most 2^26 blocks)
  if (fill)
    k12_common<true><<<slots, K12_WAVE, 0, st>>>(n_views, voff, ckey, cxy, ncom, has, size, has_rank, size_off, pts, pairs);
  else
    k12_common<false><<<slots, K12_WAVE, 0, st>>>(n_views, voff, ckey, cxy, ncom, has, size, has_rank, size_off, pts, pairs);
}
void launch_k12_samples(hipStream_t st, uint32_t p0, uint32_t n_pairs, uint32_t iterations, int32_t n_views, u64 rng_seed, const K12Pair* pairs,
                        uint32_t* idx) {
  if (!n_pairs) return;
  k12_samples<<<k12_blocks(n_pairs), K12_BLOCK, 0, st>>>(p0, n_pairs, iterations, n_views, rng_seed, pairs, idx);
}
void launch_k12_fit(hipStream_t st, uint32_t p0, uint32_t n_pairs, uint32_t iterations, const K12Pair* pairs, const float4* pts,
                    const uint32_t* idx, const K12Normal* normals, K12Fit* fits) {
  const u64 n = normals ? (u64)n_pairs : (u64)n_pairs * iterations;
  if (!n) return;
  k12_fit<<<(uint32_t)((n + K12_WAVE - 1) / K12_WAVE), K12_WAVE, 0, st>>>(p0, n_pairs, iterations, pairs, pts, idx, normals, fits);
}
void launch_k12_select(hipStream_t st, uint32_t p0, uint32_t n_pairs, uint32_t iterations, uint32_t stage_points, int32_t n_views,
                       const K12Pair* pairs, const float4* pts, const K12Fit* fits, u64* err, uint32_t* inl, K12Normal* normals, K12Sel* sel,
                       double* F, uint8_t* F_valid, u64* ctr) {
  if (!n_pairs) return;
  k12_select<<<n_pairs, K12_WAVE, (size_t)stage_points * sizeof(float4), st>>>(p0, iterations, stage_points, n_views, pairs, pts, fits, err,
                                                                               inl, normals, sel, F, F_valid, ctr);
}
void launch_k12_final(hipStream_t st, uint32_t p0, uint32_t n_pairs, int32_t n_views, const K12Pair* pairs, const float4* pts,
                      const K12Fit* refits, const K12Sel* sel, double* F) {
  if (!n_pairs) return;
  k12_final<<<n_pairs, K12_WAVE, 0, st>>>(p0, n_views, pairs, pts, refits, sel, F);
}

}  // namespace eg3d
