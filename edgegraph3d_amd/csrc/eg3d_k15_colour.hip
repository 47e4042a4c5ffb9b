// eg3d_k15_colour.hip — K15: the colours of an edge-point cloud from the source images (include/eg3d_colour.h).
//
// opc_getColorSubpix and opc_get_refpoint_mixed_color (io/output/output_point_cloud.cpp:65-105, 127-170) in two passes:
//   k15_sample  1 lane / observation  the bilinear sample (eg3d_dev_colour.h) packed into one 32-bit word; the view id, the
//                                     view's image and both coordinates are checked before any of them becomes an index,
//                                     and a failed check is recorded IN the word, so that only kept points can refuse a call
//   k15_mix     1 lane / point        the offsets checked, then the point's words read contiguously and averaged per
//                                     channel by integer division (exactly the reference's int(sum / float(n)) for
//                                     n <= 32 767: include/eg3d_colour.h states the argument)
// The images stay as uploaded, RGB8 interleaved: a sample's four taps are two runs of 6 bytes (x0, x1 adjacent but at the
// borders), read with byte loads — 12 per observation into at most two cache lines per row pair. A 4-byte pixel would make
// them 4 dword loads at the price of a conversion pass per upload and a third more HBM; not built, not measured.
// Independent of EG3D_DLT_ROWS: no geometry is computed here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_colour.h"
#include "eg3d_k15_colour.h"

namespace eg3d {

static_assert(K15_W_BAD_VIEW >> 24 == K15_BAD_VIEW && K15_W_NO_IMAGE >> 24 == K15_NO_IMAGE && K15_W_BAD_XY >> 24 == K15_BAD_XY,
              "the top byte of a word is the call's flag bits");
static_assert(255ull * EG3D_COLOUR_MAX_OBS < (1ull << 32), "a channel's sum fits 32 bits");

__global__ void __launch_bounds__(K15_BLOCK) k15_sample(K15Cloud c, const K15Image* images, int n_views, uint32_t* words) {
  const uint64_t q = (uint64_t)blockIdx.x * K15_BLOCK + threadIdx.x;
  if (q >= c.n_obs) return;
  const int32_t v = c.obs_view[q];
  const float px = c.obs_xy[2 * q], py = c.obs_xy[2 * q + 1];
  uint32_t word;
  if ((uint32_t)v >= (uint32_t)n_views) {
    word = K15_W_BAD_VIEW;
  } else {
    const K15Image im = images[v];
    if (!im.rgb)
      word = K15_W_NO_IMAGE;
    else if (!(colour_coord_ok(px) && colour_coord_ok(py)))
      word = K15_W_BAD_XY;
    else
      word = colour_sample(im.rgb, im.w, im.h, px, py);
  }
  words[q] = word;
}

__device__ __forceinline__ uint32_t k15_wave_sum(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;  // (lane 0 holds the sum)
}

__global__ void __launch_bounds__(K15_BLOCK) k15_mix(K15Cloud c, const uint32_t* words, uint8_t* rgb, uint8_t* flags,
                                                     unsigned long long* ctr) {
  const uint64_t i = (uint64_t)blockIdx.x * K15_BLOCK + threadIdx.x;
  const bool mine = i < c.n_points;
  uint32_t bad = 0, n = 0, sr = 0, sg = 0, sb = 0;
  bool kept = false;
  if (mine) {
    const uint64_t a = c.obs_off[i], b = i + 1 < c.n_points ? c.obs_off[i + 1] : c.n_obs;
    kept = !c.keep || c.keep[i] != 0;
    if (!(a <= b && b <= c.n_obs)) {
      bad = K15_BAD_OFFSETS;
    } else if (kept) {
      if (b - a > (uint64_t)EG3D_COLOUR_MAX_OBS) {
        bad = K15_LONG_LIST;
      } else {
        n = (uint32_t)(b - a);
        const uint32_t* w = words + a;
        for (uint32_t k = 0; k < n; k++) {
          const uint32_t x = w[k];
          bad |= x >> 24;
          sr += x & 0xffu;
          sg += (x >> 8) & 0xffu;
          sb += (x >> 16) & 0xffu;
        }
      }
    }
    const bool colour = kept && !bad && n;
    rgb[3 * i] = colour ? (uint8_t)(sr / n) : 0;
    rgb[3 * i + 1] = colour ? (uint8_t)(sg / n) : 0;
    rgb[3 * i + 2] = colour ? (uint8_t)(sb / n) : 0;
    if (flags) flags[i] = (kept && !bad && !n) ? (uint8_t)K15_OUT_EMPTY : 0;
    if (bad) atomicOr((uint32_t*)ctr, bad);
  }
  const bool ok = mine && kept && !bad;
  const uint32_t n_col = (uint32_t)__popcll(__ballot(ok && n)), n_emp = (uint32_t)__popcll(__ballot(ok && !n));
  const uint32_t n_obs = k15_wave_sum(ok ? n : 0u);
  if ((threadIdx.x & 63u) == 0) {
    if (n_col) atomicAdd(&ctr[1], (unsigned long long)n_col);
    if (n_emp) atomicAdd(&ctr[2], (unsigned long long)n_emp);
    if (n_obs) atomicAdd(&ctr[3], (unsigned long long)n_obs);
  }
}

void launch_k15_sample(hipStream_t st, K15Cloud c, const K15Image* images, int n_views, uint32_t* words) {
  if (!c.n_obs) return;
  hipLaunchKernelGGL(k15_sample, blocks_for(c.n_obs, K15_BLOCK), dim3(K15_BLOCK), 0, st, c, images, n_views, words);
}
void launch_k15_mix(hipStream_t st, K15Cloud c, const uint32_t* words, uint8_t* rgb, uint8_t* flags, unsigned long long* ctr) {
  if (!c.n_points) return;
  hipLaunchKernelGGL(k15_mix, blocks_for(c.n_points, K15_BLOCK), dim3(K15_BLOCK), 0, st, c, words, rgb, flags, ctr);
}

}  // namespace eg3d
