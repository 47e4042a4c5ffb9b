// eg3d_k18_nearest.hip — K18: a uniform-grid index over a point set, and the nearest distances of a second point set
// against it (include/eg3d/nearest.hpp). The arithmetic is eg3d_nearest_core.h's, shared with the host statement.
//
// Build: a grid-stride reduction of the ordered minimum / maximum (integer atomics, one set per wavefront), the cell keys,
// rocPRIM's radix sort of (key, position) — stable, so a cell's points stay in their original order —, the key-ordered
// copy of the points as 16-byte records (x, y, z, original index: one load per candidate), the heads of the cells, their
// scan, and the occupied cells' keys and starts.
//
// Query (the hot kernel): G lanes share a query, G = 1, 8 or 64, grid-stride. Every lane of a group computes the cell
// ranges and the two binary searches of a (y, z) row itself (they are the same for the group: the loads broadcast), takes
// the candidates lane, lane + G, ... of the row's contiguous run, and the group's results are combined with better() by
// G - 1 cross-lane reads. Lane 0 of a group writes d2 / nn and keeps the group's share of the figures in registers;
// at the end of the kernel a wavefront reduces them across its lanes and lane 0 issues one integer atomic per figure
// that is not at its neutral value. Integer minimum, maximum and sum give the same bits in any order. No LDS, no scratch.
// Independent of EG3D_DLT_ROWS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "eg3d_k18_nearest.h"

namespace eg3d {

using namespace nearest;
using u64 = unsigned long long;

__device__ __forceinline__ uint32_t k18_wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ uint32_t k18_wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ uint32_t k18_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  return v;
}
__device__ __forceinline__ u64 k18_wave_sum64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    v += ((u64)hi << 32) | lo;
  }
  return v;
}

__global__ void k18_init(u64* ctr, int query) {
  const int i = threadIdx.x;
  if (query) {
    if (i < K18Q_COUNT) ctr[i] = i == K18Q_MIN ? ~0ull : 0ull;
  } else {
    if (i < K18B_COUNT) ctr[i] = (i >= K18B_MIN && i < K18B_MIN + 3) ? ~0ull : 0ull;
  }
}

__global__ void __launch_bounds__(K18_BLOCK) k18_minmax(const float* X, uint64_t n, const uint8_t* keep, u64* ctr) {
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, n_dropped = 0, n_bad = 0;
  const uint64_t stride = (uint64_t)gridDim.x * K18_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * K18_BLOCK + threadIdx.x; i < n; i += stride) {
    if (keep && !keep[i]) {
      n_dropped++;
      continue;
    }
    const float x = X[3 * i], y = X[3 * i + 1], z = X[3 * i + 2];
    if (!finite3(x, y, z)) {
      n_bad++;
      continue;
    }
    const uint32_t c[3] = {ordered_code(x), ordered_code(y), ordered_code(z)};
#pragma unroll
    for (int a = 0; a < 3; a++) lo[a] = min(lo[a], c[a]), hi[a] = max(hi[a], c[a]);
  }
  // (every lane of the block arrives here: the loop has no barrier and the block is full)
  n_dropped = k18_wave_sum(n_dropped);
  n_bad = k18_wave_sum(n_bad);
#pragma unroll
  for (int a = 0; a < 3; a++) lo[a] = k18_wave_min(lo[a]), hi[a] = k18_wave_max(hi[a]);
  if ((threadIdx.x & 63u) == 0) {
    if (n_dropped) atomicAdd(&ctr[K18B_DROPPED], (u64)n_dropped);
    if (n_bad) atomicAdd(&ctr[K18B_NONFINITE], (u64)n_bad);
#pragma unroll
    for (int a = 0; a < 3; a++)
      if (lo[a] <= hi[a]) {  // (the wavefront saw a point to index)
        atomicMin(&ctr[K18B_MIN + a], (u64)lo[a]);
        atomicMax(&ctr[K18B_MAX + a], (u64)hi[a]);
      }
  }
}

__global__ void __launch_bounds__(K18_BLOCK) k18_keys(Grid g, const float* X, uint64_t n, const uint8_t* keep, u64* key, uint32_t* val) {
  const uint64_t i = (uint64_t)blockIdx.x * K18_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float x = X[3 * i], y = X[3 * i + 1], z = X[3 * i + 2];
  const bool indexed = (!keep || keep[i]) && finite3(x, y, z);
  key[i] = indexed ? point_key(g, x, y, z) : kUnindexed;
  val[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(K18_BLOCK) k18_gather(const float* X, const u64* key_sorted, const uint32_t* val_sorted, uint64_t n_indexed,
                                                        Pt* pts, uint32_t* head) {
  const uint64_t k = (uint64_t)blockIdx.x * K18_BLOCK + threadIdx.x;
  if (k > n_indexed) return;
  if (k == n_indexed) {
    head[k] = 0u;
    return;
  }
  const uint32_t j = val_sorted[k];
  Pt p;
  p.x = X[3 * (uint64_t)j], p.y = X[3 * (uint64_t)j + 1], p.z = X[3 * (uint64_t)j + 2], p.j = j;
  pts[k] = p;
  head[k] = (k == 0 || key_sorted[k] != key_sorted[k - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(K18_BLOCK) k18_cells(const u64* key_sorted, const uint32_t* head, const uint32_t* rank, uint64_t n_indexed,
                                                       u64* cell_key, uint32_t* cell_start) {
  const uint64_t k = (uint64_t)blockIdx.x * K18_BLOCK + threadIdx.x;
  if (k > n_indexed) return;
  if (k == n_indexed) {
    cell_start[rank[k]] = (uint32_t)n_indexed;  // rank[n_indexed] = n_cells <= n_indexed: inside the n_indexed + 1 entries
  } else if (head[k]) {
    cell_key[rank[k]] = key_sorted[k];
    cell_start[rank[k]] = (uint32_t)k;
  }
}

__global__ void __launch_bounds__(K18_BLOCK) k18_max_cell(const uint32_t* cell_start, uint32_t n_cells, u64* ctr) {
  uint32_t m = 0;
  const uint64_t stride = (uint64_t)gridDim.x * K18_BLOCK;
  for (uint64_t c = (uint64_t)blockIdx.x * K18_BLOCK + threadIdx.x; c < n_cells; c += stride) m = max(m, cell_start[c + 1] - cell_start[c]);
  m = k18_wave_max(m);
  if ((threadIdx.x & 63u) == 0 && m) atomicMax(&ctr[K18B_MAXCELL], (u64)m);
}

template <int G>
__global__ void __launch_bounds__(K18_BLOCK) k18_query(Grid g, const float* X, uint64_t n, const uint8_t* keep, float max_dist, K18Thresholds t,
                                                       float* d2_out, uint32_t* nn_out, u64* ctr) {
  const float md2 = max_dist * max_dist;
  const uint32_t sub = threadIdx.x & (uint32_t)(G - 1);
  const uint64_t n_groups = (uint64_t)gridDim.x * (K18_BLOCK / G);
  uint32_t n_dropped = 0, n_bad = 0, n_within = 0, lo = 0xffffffffu, hi = 0u, below[kMaxThresholds];
  u64 sum = 0;
#pragma unroll
  for (int k = 0; k < kMaxThresholds; k++) below[k] = 0u;
  // (a group's lanes share q, so they stay in the loop together: the cross-lane reads below meet only active lanes)
  for (uint64_t q = (uint64_t)blockIdx.x * (K18_BLOCK / G) + threadIdx.x / G; q < n; q += n_groups) {
    float bd = bits_f32(kInfBits);
    uint32_t bj = kNone;
    const bool dropped = keep && !keep[q];
    const float qx = X[3 * q], qy = X[3 * q + 1], qz = X[3 * q + 2];
    const bool bad = !dropped && !finite3(qx, qy, qz);
    if (!dropped && !bad) {
      search(g, qx, qy, qz, max_dist, md2, sub, (uint32_t)G, &bd, &bj);
#pragma unroll
      for (int o = G >> 1; o > 0; o >>= 1) {
        const float od = __shfl_xor(bd, o);
        const uint32_t oj = (uint32_t)__shfl_xor((int)bj, o);
        if (better(od, oj, bd, bj)) bd = od, bj = oj;
      }
    }
    if (sub == 0) {
      d2_out[q] = bd;
      if (nn_out) nn_out[q] = bj;
      n_dropped += dropped ? 1u : 0u;
      n_bad += bad ? 1u : 0u;
      if (bj != kNone) {
        const uint32_t b = f32_bits(bd);
        n_within++;
        lo = min(lo, b);
        hi = max(hi, b);
        sum += quantise(bd, max_dist);
#pragma unroll
        for (int k = 0; k < kMaxThresholds; k++) below[k] += bd < t.t2[k] ? 1u : 0u;
      }
    }
  }
  n_dropped = k18_wave_sum(n_dropped);
  n_bad = k18_wave_sum(n_bad);
  n_within = k18_wave_sum(n_within);
  if (n_dropped && (threadIdx.x & 63u) == 0) atomicAdd(&ctr[K18Q_DROPPED], (u64)n_dropped);
  if (n_bad && (threadIdx.x & 63u) == 0) atomicAdd(&ctr[K18Q_NONFINITE], (u64)n_bad);
  if (!n_within) return;  // (wave-uniform: the sum is every lane's)
  lo = k18_wave_min(lo);
  hi = k18_wave_max(hi);
  sum = k18_wave_sum64(sum);
#pragma unroll
  for (int k = 0; k < kMaxThresholds; k++) below[k] = k18_wave_sum(below[k]);
  if ((threadIdx.x & 63u) == 0) {
    atomicAdd(&ctr[K18Q_WITHIN], (u64)n_within);
    atomicMin(&ctr[K18Q_MIN], (u64)lo);
    atomicMax(&ctr[K18Q_MAX], (u64)hi);
    if (sum) atomicAdd(&ctr[K18Q_SUM], sum);
#pragma unroll
    for (int k = 0; k < kMaxThresholds; k++)
      if (below[k]) atomicAdd(&ctr[K18Q_BELOW + k], (u64)below[k]);
  }
}

__global__ void k18_median(const uint32_t* d2_sorted, u64* ctr) {
  const u64 w = ctr[K18Q_WITHIN];
  ctr[K18Q_MEDIAN] = w ? (u64)d2_sorted[(w - 1) / 2] : (u64)kInfBits;  // (w <= n: the within set is part of the sorted array)
}

static unsigned k18_blocks(uint64_t threads, unsigned cap) {
  return (unsigned)std::min<uint64_t>((threads + K18_BLOCK - 1) / K18_BLOCK, cap);
}

void launch_k18_init(hipStream_t st, u64* ctr, bool query) { hipLaunchKernelGGL(k18_init, dim3(1), dim3(64), 0, st, ctr, query ? 1 : 0); }

void launch_k18_minmax(hipStream_t st, const float* X, uint64_t n, const uint8_t* keep, u64* ctr) {
  if (!n) return;
  hipLaunchKernelGGL(k18_minmax, dim3(k18_blocks(n, K18_MAX_BLOCKS)), dim3(K18_BLOCK), 0, st, X, n, keep, ctr);
}

void launch_k18_keys(hipStream_t st, Grid g, const float* X, uint64_t n, const uint8_t* keep, u64* key, uint32_t* val) {
  if (!n) return;  // (n < 2^32: at most 2^24 blocks)
  hipLaunchKernelGGL(k18_keys, dim3(k18_blocks(n, 0xffffffffu)), dim3(K18_BLOCK), 0, st, g, X, n, keep, key, val);
}

void launch_k18_gather(hipStream_t st, const float* X, const u64* key_sorted, const uint32_t* val_sorted, uint64_t n_indexed, Pt* pts,
                       uint32_t* head) {
  hipLaunchKernelGGL(k18_gather, dim3(k18_blocks(n_indexed + 1, 0xffffffffu)), dim3(K18_BLOCK), 0, st, X, key_sorted, val_sorted, n_indexed,
                     pts, head);
}

void launch_k18_cells(hipStream_t st, const u64* key_sorted, const uint32_t* head, const uint32_t* rank, uint64_t n_indexed, u64* cell_key,
                      uint32_t* cell_start) {
  hipLaunchKernelGGL(k18_cells, dim3(k18_blocks(n_indexed + 1, 0xffffffffu)), dim3(K18_BLOCK), 0, st, key_sorted, head, rank, n_indexed,
                     cell_key, cell_start);
}

void launch_k18_max_cell(hipStream_t st, const uint32_t* cell_start, uint32_t n_cells, u64* ctr) {
  if (!n_cells) return;
  hipLaunchKernelGGL(k18_max_cell, dim3(k18_blocks(n_cells, K18_MAX_BLOCKS)), dim3(K18_BLOCK), 0, st, cell_start, n_cells, ctr);
}

void launch_k18_query(hipStream_t st, int group, Grid g, const float* X, uint64_t n, const uint8_t* keep, float max_dist, K18Thresholds t,
                      float* d2_out, uint32_t* nn_out, u64* ctr) {
  if (!n) return;
  const dim3 grid(k18_blocks(n * (uint64_t)group, K18_MAX_BLOCKS)), block(K18_BLOCK);
  if (group == 64)
    hipLaunchKernelGGL(k18_query<64>, grid, block, 0, st, g, X, n, keep, max_dist, t, d2_out, nn_out, ctr);
  else if (group == 8)
    hipLaunchKernelGGL(k18_query<8>, grid, block, 0, st, g, X, n, keep, max_dist, t, d2_out, nn_out, ctr);
  else
    hipLaunchKernelGGL(k18_query<1>, grid, block, 0, st, g, X, n, keep, max_dist, t, d2_out, nn_out, ctr);
}

void launch_k18_median(hipStream_t st, const uint32_t* d2_sorted, u64* ctr) {
  hipLaunchKernelGGL(k18_median, dim3(1), dim3(1), 0, st, d2_sorted, ctr);
}

hipError_t k18_sort_bits(hipStream_t st, void* tmp, size_t& tmp_bytes, const uint32_t* in, uint32_t* out, size_t n) {
  return rocprim::radix_sort_keys(tmp, tmp_bytes, in, out, n, 0, 32, st);
}

}  // namespace eg3d
