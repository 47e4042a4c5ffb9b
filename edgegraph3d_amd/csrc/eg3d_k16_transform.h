// Host-visible declarations of K16 (eg3d_k16_transform.hip): a 4 x 4 transform applied to the points of a cloud
// (include/eg3d_transform.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_kernels.h"

namespace eg3d {

#define K16_BLOCK 256
// the grid's cap: 256 CUs x 8 workgroups of four wavefronts = 8 wavefronts per SIMD; a wavefront loops over its tiles of 64
// points, so that the call's two counts cost at most one atomic per wavefront and not one per 64 points
#define K16_MAX_BLOCKS 2048

// M[i][j] = (float)T[4 i + j], passed BY VALUE: the 16 values arrive as kernel arguments and stay in scalar registers
struct K16Mat {
  float m[4][4];
};

// One lane per point: X_out[i] = the point transform of X[i] (include/eg3d_host_transform.h, "Points") where keep is null
// or keep[i] != 0, the bits of X[i] otherwise. X_out == X is allowed; a partial overlap is the caller's to refuse. Neither
// array needs more than the 4-byte alignment of a float. ctr[0] += points the mask drops, ctr[1] += kept points whose result
// has a component that is not finite (one atomic per wave each, none for a wave whose count is zero).
void launch_k16_transform(hipStream_t st, K16Mat M, const float* X, uint64_t n_points, const uint8_t* keep, float* X_out,
                          unsigned long long* ctr);

}  // namespace eg3d
