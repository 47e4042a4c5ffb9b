// eg3d_k7_dedup.hip — K7 (gfx950): the 3 px de-duplication of a device-resident cloud (k7_dedup_claim, k7_dedup_keep).
// All arithmetic follows the contract in DESIGN.md (no FMA contraction: -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_pipeline.h"
#include "eg3d_kernels.h"

namespace eg3d {

// ------------------------------------------------------------------ K7 ---------
// The 3 px de-duplication of a device-resident cloud (filter_3d_points_close_2d_array; eg3d_host_filter_close_2d is the
// sequential statement). The first point that touches a cell is always kept (nothing before it occupied the cell), so a
// cell is occupied before point i exactly when a point before i has an observation in it, and
//   keep[i] = some observation of i lies in a valid cell whose SMALLEST touching point index is i.
// Two order-independent passes over a claim map first[n_views x w x h] of point indices (0xFFFFFFFF = untouched):
//   k7_dedup_claim  1 lane / observation: atomicMin(first[cell], index_base + owning point)
//   k7_dedup_keep   8 lanes / point: keep = any observation whose cell holds index_base + point; kept points counted
// The outcome of atomicMin does not depend on arrival order, so the mask is deterministic. Claims persist between calls:
// with index_base = the number of points of the earlier clouds, a cloud is deduplicated against all of them.
// The cell of an observation as cell_of in host/post_steps.cpp: a true float division (correctly rounded in this build),
// the range test written so that NaN fails, truncation toward zero (a coordinate in (-3, 0) lands in cell 0), the range
// test again on the integers. Returns false for an observation without a cell.
__device__ __forceinline__ bool k7_cell(const K7Map& m, int32_t v, float x, float y, uint64_t* cell) {
  const float fx = x / 3.0f, fy = y / 3.0f;
  if (v < 0 || v >= m.n_views || !(fx > -1.0f) || !(fy > -1.0f) || !(fx < (float)m.w) || !(fy < (float)m.h)) return false;
  const int cx = (int)fx, cy = (int)fy;
  if (cx < 0 || cy < 0 || cx >= m.w || cy >= m.h) return false;
  *cell = ((uint64_t)v * (uint64_t)m.h + (uint64_t)cy) * (uint64_t)m.w + (uint64_t)cx;
  return true;
}
// The last point of [lo, hi) whose offset is <= j (lo's is): the owner of observation j, empty lists before it skipped.
// Reads obs_off inside [lo, hi) only, whatever the offsets hold.
__device__ __forceinline__ uint64_t k7_owner(const eg3d_off_t* obs_off, uint64_t lo, uint64_t hi, uint64_t j) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (obs_off[mid] <= j)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
// Adjacent lanes take adjacent observations: obs_view and the 8-byte (x, y) words load coalesced. The owning point: the
// wave searches the whole offset array once for its first observation (every lane the same addresses), stages the next
// 64 offsets in LDS, and a lane counts how many of them are <= its observation (6 LDS probes). A wave's 64 observations
// span more than 64 points only across empty lists; such a lane falls back to the search over the whole array.
__global__ void __launch_bounds__(K7_BLOCK) k7_dedup_claim(CloudView in, K7Map m, uint32_t index_base) {
  __shared__ uint64_t s_off[K7_BLOCK / 64][64];
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u;
  const uint64_t j0 = (uint64_t)blockIdx.x * K7_BLOCK + (uint64_t)w * 64, j = j0 + lane;
  uint64_t p0 = 0;
  if (j0 < in.n_obs) {
    p0 = k7_owner(in.obs_off, 0, in.n_points, j0);
    const uint64_t q = p0 + 1 + lane;
    s_off[w][lane] = q < in.n_points ? in.obs_off[q] : ~0ull;
  }
  __syncthreads();
  if (j >= in.n_obs) return;
  uint32_t lo = 0, hi = 64;  // the number of staged offsets <= j
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (s_off[w][mid] <= j)
      lo = mid + 1;
    else
      hi = mid;
  }
  uint64_t p = p0 + lo;
  if (lo == 64) p = k7_owner(in.obs_off, p, in.n_points, j);
  if (p == 0 && in.obs_off[0] > j) return;  // (an observation in front of the first list belongs to no point)
  const int32_t v = in.obs_view[j];
  const unsigned long long xy = *(const unsigned long long*)(in.obs_xy + 2 * j);
  uint64_t cell;
  if (!k7_cell(m, v, __uint_as_float((uint32_t)xy), __uint_as_float((uint32_t)(xy >> 32)), &cell)) return;
  const uint32_t id = index_base + (uint32_t)p;
  // most observations are not the first of their cell: an entry only ever decreases, so one that already reads <= id
  // cannot be lowered by this lane and the atomic is skipped (measured: DESIGN_LOG.md, "Dedup on the device")
  if (m.first[cell] <= id) return;
  atomicMin(m.first + cell, id);
}
// 8 lanes per point, 32 points per block: the lists of a C2 / C3' cloud hold 3 to 9 observations, so a group covers its
// list in one or two strides, the 8 groups of a wave read 8 adjacent lists (one contiguous stretch of obs_view / obs_xy),
// and the verdict is one ballot. Against 1 lane / observation + a per-point OR this needs no second owner search and no
// zeroed mask, and writes every byte of the mask exactly once; against 1 lane / point its loads are contiguous per wave
// rather than strided by list. A list that is not an ascending range inside [0, n_obs] raises K5_FLAG_BAD_OFFSETS and
// drops its point. Kept points: ballot + popcount per wave, LDS per block, one atomic per block.
__global__ void __launch_bounds__(K7_BLOCK) k7_dedup_keep(CloudView in, K7Map m, uint32_t index_base, uint8_t* keep,
                                                         unsigned long long* n_kept, uint32_t* flags) {
  __shared__ uint32_t s_n[K7_BLOCK / 64];
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u, sub = lane & 7u;
  const uint64_t i = (uint64_t)blockIdx.x * (K7_BLOCK / 8) + (t >> 3);
  bool hit = false;
  if (i < in.n_points) {
    const uint64_t a = in.obs_off[i], b = i + 1 < in.n_points ? in.obs_off[i + 1] : in.n_obs;
    if (!(a <= b && b <= in.n_obs)) {
      if (sub == 0) atomicOr(flags, K5_FLAG_BAD_OFFSETS);
    } else {
      const uint32_t id = index_base + (uint32_t)i;
      for (uint64_t j = a + sub; j < b && !hit; j += 8) {
        const int32_t v = in.obs_view[j];
        const unsigned long long xy = *(const unsigned long long*)(in.obs_xy + 2 * j);
        uint64_t cell;
        if (k7_cell(m, v, __uint_as_float((uint32_t)xy), __uint_as_float((uint32_t)(xy >> 32)), &cell)) hit = m.first[cell] == id;
      }
    }
  }
  const unsigned long long any = __ballot(hit);
  const bool kept = ((any >> (lane & ~7u)) & 0xffull) != 0;
  if (sub == 0 && i < in.n_points) keep[i] = kept ? 1 : 0;
  const uint32_t n = (uint32_t)__popcll(__ballot(kept && sub == 0));
  if (lane == 0) s_n[w] = n;
  __syncthreads();
  if (t == 0) {
    uint32_t sum = 0;
    for (uint32_t q = 0; q < K7_BLOCK / 64; q++) sum += s_n[q];
    if (sum) atomicAdd(n_kept, (unsigned long long)sum);
  }
}

void launch_dedup_claim(hipStream_t st, CloudView in, K7Map m, uint32_t index_base) {
  if (!in.n_points || !in.n_obs) return;
  hipLaunchKernelGGL(k7_dedup_claim, blocks_for(in.n_obs, K7_BLOCK), dim3(K7_BLOCK), 0, st, in, m, index_base);
}
void launch_dedup_keep(hipStream_t st, CloudView in, K7Map m, uint32_t index_base, uint8_t* keep, unsigned long long* n_kept,
                       uint32_t* flags) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k7_dedup_keep, blocks_for(in.n_points, K7_BLOCK / 8), dim3(K7_BLOCK), 0, st, in, m, index_base, keep,
                     n_kept, flags);
}

}  // namespace eg3d
