// eg3d_k16_transform.hip — K16: a 4 x 4 transform applied to the points of a cloud (include/eg3d_transform.h).
//
// transform_3d_point (coordinate_system_transform/transform_coordinate_system.cpp:152-155) with one lane per point. A
// point is 12 bytes, so the 64 points of a TILE are 768 contiguous bytes of the flat array: 48 whole 16-byte words when the
// array starts on a 16-byte boundary, 49 with a partial first and last one when it starts 4, 8 or 12 bytes past one. A
// wavefront takes one tile after the other (tile, tile + waves of the grid, ...):
//   load     lane w < 49 reads word w with ONE 128-bit load; a word that is only partly this tile's (the array's ragged
//            ends, the words neighbouring tiles of a misaligned array share) is read float by float, and only the floats
//            of the tile's own points: nothing outside [X, X + 3 n) is ever addressed, and in place no wavefront reads
//            what another one writes
//   gather   lane l takes its three floats out of the word registers (4 cross-lane reads per float, one per word
//            component, and a select)
//   compute  the sums and the three divisions in the order of include/eg3d_host_transform.h; the matrix is a kernel
//            argument and stays in scalar registers
//   scatter  the reverse of gather with the OUTPUT array's own misalignment, then one 128-bit store per whole word
// The two counts — points the mask DROPS, non-finite results — are kept per wavefront over all its tiles (ballots) and
// added to the call's with one atomic each at the end, and only when they are not zero: a call without a mask and without
// a non-finite result issues no atomic at all. Additions to one address serialise at some 13 ns each: one per tile —
// 875 000 for a 56 M-point cloud — took 10.5 ms where the data move in a fraction of that, and even one per wavefront of
// the capped grid (8192, of the KEPT points, which are never zero) was most of a 1.7 M-point call (DESIGN_LOG.md, "K16").
// No LDS, no scratch. Independent of EG3D_DLT_ROWS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "eg3d_k16_transform.h"

namespace eg3d {

__device__ __forceinline__ float k16_pick4(uint32_t c, float a0, float a1, float a2, float a3) {
  return c == 0 ? a0 : c == 1 ? a1 : c == 2 ? a2 : a3;
}
__device__ __forceinline__ bool k16_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// One tile: the `cnt` (1 .. 64) points that start at xin / xout, `keep` at the tile's first point or null. mi, mo: how
// many floats past a 16-byte boundary xin / xout start (0 .. 3). Every lane of the wavefront must call it together.
__device__ __forceinline__ void k16_tile(const K16Mat& M, uint32_t lane, const float* xin, float* xout, const uint8_t* keep,
                                         int32_t cnt, int32_t mi, int32_t mo, uint32_t& n_dropped, uint32_t& n_bad) {
  const int32_t nf = 3 * cnt;  // the tile's floats
  // ---- load: word `lane` of the aligned words that cover xin[0 .. nf)
  float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
  {
    const int32_t q = 4 * (int32_t)lane - mi;  // index in xin of the word's first float
    if (q >= 0 && q + 3 < nf) {
      const float4 v = *reinterpret_cast<const float4*>(xin + q);
      w0 = v.x, w1 = v.y, w2 = v.z, w3 = v.w;
    } else {
      if (q >= 0 && q < nf) w0 = xin[q];
      if (q + 1 >= 0 && q + 1 < nf) w1 = xin[q + 1];
      if (q + 2 >= 0 && q + 2 < nf) w2 = xin[q + 2];
      if (q + 3 >= 0 && q + 3 < nf) w3 = xin[q + 3];
    }
  }
  // ---- gather: every lane takes part in the cross-lane reads, its point or not
  float p[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint32_t f = 3u * lane + (uint32_t)mi + (uint32_t)k;  // <= 194: word <= 48
    const int src = (int)(f >> 2);
    p[k] = k16_pick4(f & 3u, __shfl(w0, src), __shfl(w1, src), __shfl(w2, src), __shfl(w3, src));
  }
  // ---- compute
  const bool mine = (int32_t)lane < cnt;
  const bool kept = mine && (!keep || keep[lane] != 0);
  float o0 = p[0], o1 = p[1], o2 = p[2];  // (a point the mask drops keeps its bits)
  if (kept) {
    const float x = p[0], y = p[1], z = p[2], w = 1.0f;
    const float h0 = ((M.m[0][0] * x + M.m[0][1] * y) + M.m[0][2] * z) + M.m[0][3] * w;
    const float h1 = ((M.m[1][0] * x + M.m[1][1] * y) + M.m[1][2] * z) + M.m[1][3] * w;
    const float h2 = ((M.m[2][0] * x + M.m[2][1] * y) + M.m[2][2] * z) + M.m[2][3] * w;
    const float h3 = ((M.m[3][0] * x + M.m[3][1] * y) + M.m[3][2] * z) + M.m[3][3] * w;
    o0 = h0 / h3;
    o1 = h1 / h3;
    o2 = h2 / h3;
  }
  const bool bad = kept && (k16_nonfinite(o0) || k16_nonfinite(o1) || k16_nonfinite(o2));
  n_dropped += (uint32_t)__popcll(__ballot(mine && !kept));  // (wave-uniform: every lane adds the same counts)
  n_bad += (uint32_t)__popcll(__ballot(bad));
  // ---- scatter: word `lane` of the aligned words that cover xout[0 .. nf)
  const int32_t q0 = 4 * (int32_t)lane - mo;
  float s[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int32_t q = q0 + c;
    const uint32_t qq = (q >= 0 && q < nf) ? (uint32_t)q : 0u;  // (a float that is not ours: any lane, the value is not stored)
    const uint32_t pl = qq / 3u, pc = qq - 3u * pl;
    const float a0 = __shfl(o0, (int)pl), a1 = __shfl(o1, (int)pl), a2 = __shfl(o2, (int)pl);
    s[c] = pc == 0 ? a0 : pc == 1 ? a1 : a2;
  }
  if (q0 >= 0 && q0 + 3 < nf) {
    *reinterpret_cast<float4*>(xout + q0) = make_float4(s[0], s[1], s[2], s[3]);
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (q0 + c >= 0 && q0 + c < nf) xout[q0 + c] = s[c];
  }
}

__global__ void __launch_bounds__(K16_BLOCK) k16_transform(K16Mat M, const float* X, uint64_t n_points, const uint8_t* keep,
                                                           float* X_out, unsigned long long* ctr) {
  const uint32_t lane = threadIdx.x & 63u;
  const int32_t mi = (int32_t)(((uintptr_t)X >> 2) & 3u), mo = (int32_t)(((uintptr_t)X_out >> 2) & 3u);
  const uint64_t n_tiles = (n_points + 63u) >> 6, n_waves = (uint64_t)gridDim.x * (K16_BLOCK / 64);
  uint32_t n_dropped = 0, n_bad = 0;  // (a wavefront of the capped grid sees fewer than 2^32 points for any n_points below 2^45)
  for (uint64_t tile = (uint64_t)blockIdx.x * (K16_BLOCK / 64) + (threadIdx.x >> 6); tile < n_tiles; tile += n_waves) {
    const uint64_t base = tile << 6;  // (3 * base is a multiple of 192 floats: the tile is as misaligned as the array itself)
    const int32_t cnt = (int32_t)(n_points - base < 64 ? n_points - base : 64);
    k16_tile(M, lane, X + 3 * base, X_out + 3 * base, keep ? keep + base : nullptr, cnt, mi, mo, n_dropped, n_bad);
  }
  if (lane == 0) {
    if (n_dropped) atomicAdd(&ctr[0], (unsigned long long)n_dropped);
    if (n_bad) atomicAdd(&ctr[1], (unsigned long long)n_bad);
  }
}

void launch_k16_transform(hipStream_t st, K16Mat M, const float* X, uint64_t n_points, const uint8_t* keep, float* X_out,
                          unsigned long long* ctr) {
  if (!n_points) return;
  const unsigned blocks = std::min<uint64_t>((n_points + K16_BLOCK - 1) / K16_BLOCK, K16_MAX_BLOCKS);
  hipLaunchKernelGGL(k16_transform, dim3(blocks), dim3(K16_BLOCK), 0, st, M, X, n_points, keep, X_out, ctr);
}

}  // namespace eg3d
