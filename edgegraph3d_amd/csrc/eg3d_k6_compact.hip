// eg3d_k6_compact.hip — K6 (gfx950): order-preserving stream compaction of a device-resident cloud
// (k6_compact_count, k6_compact_scan, k6_compact_scatter).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_pipeline.h"
#include "eg3d_dev_coopgn.h"
#include "eg3d_kernels.h"

namespace eg3d {

// ------------------------------------------------------------------ K6 ---------
// Order-preserving stream compaction of a device-resident cloud (all seven arrays), three launches:
//   k6_compact_count    1 lane / point, K6_BLOCK points per block: surviving points and observations of the block
//   k6_compact_scan     one workgroup: exclusive scan of the block totals, both columns 64-bit, totals appended
//   k6_compact_scatter  1 WAVE / 64 source points (shaped like k4_emit): __ballot + popcount rank the surviving points,
//                       wave_incl_scan gives their observation offsets; then the lanes stride over the wave's contiguous
//                       DESTINATION observation range and each finds its source point by a binary search over the <= 64
//                       offsets the wave holds in LDS — the stores of the five observation arrays are coalesced rows, the
//                       loads are coalesced within every surviving list.
// A list that is not an ascending range inside [0, n_obs], or longer than K5_MAX_LIST, drops its point and raises
// K5_FLAG_BAD_OFFSETS in the count pass (the host then fails the call before anything is scattered).
struct K6Pt {
  bool surv;
  uint32_t k;
  uint64_t a;
};
__device__ __forceinline__ K6Pt k6_point(const CloudView& in, const uint8_t* keep, int32_t min_obs, uint64_t i, bool* bad) {
  K6Pt p{false, 0, 0};
  if (i >= in.n_points) return p;
  const uint64_t a = in.obs_off[i], b = i + 1 < in.n_points ? in.obs_off[i + 1] : in.n_obs;
  if (!(a <= b && b <= in.n_obs && b - a <= (uint64_t)K5_MAX_LIST)) {
    *bad = true;
    return p;
  }
  p.a = a;
  p.k = (uint32_t)(b - a);
  p.surv = (!keep || keep[i]) && (min_obs < 0 || p.k > (uint32_t)min_obs);
  return p;
}
__global__ void __launch_bounds__(K6_BLOCK) k6_compact_count(CloudView in, const uint8_t* keep, int32_t min_obs,
                                                            unsigned long long* blk, uint32_t* flags) {
  __shared__ uint32_t s_p[K6_BLOCK / 64], s_o[K6_BLOCK / 64];
  const uint32_t t = threadIdx.x, w = t >> 6;
  bool bad = false;
  const K6Pt p = k6_point(in, keep, min_obs, (uint64_t)blockIdx.x * K6_BLOCK + t, &bad);
  if (bad) atomicOr(flags, K5_FLAG_BAD_OFFSETS);
  const uint32_t np = (uint32_t)__popcll(__ballot(p.surv));
  const uint32_t no = lane_bcast((uint32_t)wave_incl_scan((int)(p.surv ? p.k : 0u)), 63);  // <= 64 x 2^24
  if ((t & 63u) == 0) {
    s_p[w] = np;
    s_o[w] = no;
  }
  __syncthreads();
  if (t == 0) {
    unsigned long long sp = 0, so = 0;
    for (uint32_t q = 0; q < K6_BLOCK / 64; q++) {
      sp += s_p[q];
      so += s_o[q];
    }
    blk[2 * (uint64_t)blockIdx.x] = sp;
    blk[2 * (uint64_t)blockIdx.x + 1] = so;
  }
}
__device__ __forceinline__ unsigned long long wave_incl_scan_u64(unsigned long long v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long u = __shfl_up(v, d, 64);
    if (lane >= (uint32_t)d) v += u;
  }
  return v;
}
__global__ void __launch_bounds__(1024) k6_compact_scan(uint64_t n_blocks, unsigned long long* blk) {
  __shared__ unsigned long long s_p[16], s_o[16];
  const uint32_t t = threadIdx.x, w = t >> 6;
  unsigned long long base_p = 0, base_o = 0;
  for (uint64_t c0 = 0; c0 < n_blocks; c0 += 1024) {
    const uint64_t i = c0 + t;
    const unsigned long long vp = i < n_blocks ? blk[2 * i] : 0, vo = i < n_blocks ? blk[2 * i + 1] : 0;
    const unsigned long long ip = wave_incl_scan_u64(vp), io = wave_incl_scan_u64(vo);
    if ((t & 63u) == 63u) {
      s_p[w] = ip;
      s_o[w] = io;
    }
    __syncthreads();
    unsigned long long pre_p = 0, pre_o = 0, tot_p = 0, tot_o = 0;
    for (uint32_t q = 0; q < 16; q++) {
      if (q < w) {
        pre_p += s_p[q];
        pre_o += s_o[q];
      }
      tot_p += s_p[q];
      tot_o += s_o[q];
    }
    if (i < n_blocks) {
      blk[2 * i] = base_p + pre_p + ip - vp;
      blk[2 * i + 1] = base_o + pre_o + io - vo;
    }
    base_p += tot_p;
    base_o += tot_o;
    __syncthreads();
  }
  if (t == 0) {
    blk[2 * n_blocks] = base_p;
    blk[2 * n_blocks + 1] = base_o;
  }
}
template <bool NT, typename T>
__device__ __forceinline__ T k6_load(const T* p) {
  if constexpr (NT)
    return __builtin_nontemporal_load(p);
  else
    return *p;
}
template <bool NT>
__global__ void __launch_bounds__(K6_BLOCK) k6_compact_scatter(CloudView in, const uint8_t* keep, const float* X_new,
                                                              int32_t min_obs, const unsigned long long* blk, CloudOut out) {
  __shared__ uint32_t s_p[K6_BLOCK / 64], s_o[K6_BLOCK / 64];
  __shared__ uint32_t s_incl[K6_BLOCK / 64][64];  // inclusive sums of the surviving lists of the wave's points
  __shared__ uint64_t s_src[K6_BLOCK / 64][64];   // first source observation of the point minus its exclusive sum
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u;
  const uint64_t i = (uint64_t)blockIdx.x * K6_BLOCK + t;
  bool bad = false;
  const K6Pt p = k6_point(in, keep, min_obs, i, &bad);
  const unsigned long long mask = __ballot(p.surv);
  const uint32_t prank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
  const uint32_t ks = p.surv ? p.k : 0u;
  const uint32_t incl = (uint32_t)wave_incl_scan((int)ks);
  const uint32_t wave_obs = lane_bcast(incl, 63);
  s_incl[w][lane] = incl;
  s_src[w][lane] = p.a - (uint64_t)(incl - ks);
  if (lane == 0) {
    s_p[w] = (uint32_t)__popcll(mask);
    s_o[w] = wave_obs;
  }
  __syncthreads();
  uint64_t pbase = blk[2 * (uint64_t)blockIdx.x], obase = blk[2 * (uint64_t)blockIdx.x + 1];
  for (uint32_t q = 0; q < w; q++) {
    pbase += s_p[q];
    obase += s_o[q];
  }
  if (p.surv) {
    const uint64_t d = pbase + prank;
    const float* xs = X_new ? X_new : in.X;
    out.X[3 * d] = k6_load<NT>(xs + 3 * i);
    out.X[3 * d + 1] = k6_load<NT>(xs + 3 * i + 1);
    out.X[3 * d + 2] = k6_load<NT>(xs + 3 * i + 2);
    out.obs_off[d] = obase + (incl - ks);
    out.key[4 * d] = k6_load<NT>(in.key + 4 * i);
    out.key[4 * d + 1] = k6_load<NT>(in.key + 4 * i + 1);
    out.key[4 * d + 2] = k6_load<NT>(in.key + 4 * i + 2);
    out.key[4 * d + 3] = k6_load<NT>(in.key + 4 * i + 3);
  }
  for (uint32_t f = lane; f < wave_obs; f += 64) {
    uint32_t lo = 0, hi = 63;  // the first lane whose inclusive sum exceeds f (it exists: f < s_incl[w][63])
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s_incl[w][mid] > f)
        hi = mid;
      else
        lo = mid + 1;
    }
    const uint64_t so = s_src[w][lo] + f, o = obase + f;
    out.obs_view[o] = k6_load<NT>(in.obs_view + so);
    out.obs_pl[o] = k6_load<NT>(in.obs_pl + so);
    out.obs_seg[o] = k6_load<NT>(in.obs_seg + so);
    *(unsigned long long*)(out.obs_xy + 2 * o) = k6_load<NT>((const unsigned long long*)(in.obs_xy + 2 * so));  // (x, y) as one 8-byte word
  }
}

void launch_compact_count(hipStream_t st, CloudView in, const uint8_t* keep, int32_t min_obs, unsigned long long* blk,
                          uint32_t* flags) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k6_compact_count, blocks_for(in.n_points, K6_BLOCK), dim3(K6_BLOCK), 0, st, in, keep, min_obs, blk, flags);
}
void launch_compact_scan(hipStream_t st, uint64_t n_blocks, unsigned long long* blk) {
  hipLaunchKernelGGL(k6_compact_scan, dim3(1), dim3(1024), 0, st, n_blocks, blk);
}
void launch_compact_scatter(hipStream_t st, CloudView in, const uint8_t* keep, const float* X_new, int32_t min_obs,
                            const unsigned long long* blk, CloudOut out, bool nt) {
  if (!in.n_points) return;
  if (nt)
    hipLaunchKernelGGL(k6_compact_scatter<true>, blocks_for(in.n_points, K6_BLOCK), dim3(K6_BLOCK), 0, st, in, keep, X_new,
                       min_obs, blk, out);
  else
    hipLaunchKernelGGL(k6_compact_scatter<false>, blocks_for(in.n_points, K6_BLOCK), dim3(K6_BLOCK), 0, st, in, keep, X_new,
                       min_obs, blk, out);
}

}  // namespace eg3d
