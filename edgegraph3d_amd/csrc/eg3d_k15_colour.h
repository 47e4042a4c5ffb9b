// Host-visible declarations of K15 (eg3d_k15_colour.hip): the colours of a cloud from the source images
// (include/eg3d_colour.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_kernels.h"

namespace eg3d {

#define K15_BLOCK 256
// flag word of the call (ctr[0]): what the observation words of the KEPT points carried, and what the offsets showed
#define K15_BAD_VIEW 1u    /* a view id outside [0, n_views) */
#define K15_NO_IMAGE 2u    /* a view for which no image was uploaded */
#define K15_BAD_XY 4u      /* a coordinate that is not finite, or of magnitude >= 1e7 */
#define K15_BAD_OFFSETS 8u /* a list that is not an ascending range inside [0, n_obs] (any point, kept or not) */
#define K15_LONG_LIST 16u  /* a kept point with more than 32 767 observations */

#define K15_OUT_EMPTY 1u /* (= EG3D_COLOUR_FLAG_EMPTY: eg3d_api_colour.hip asserts it) */

// one view's image on the device: RGB8 interleaved, row-major; rgb == nullptr: the view has none
struct K15Image {
  const uint8_t* rgb;
  int32_t w, h;
};

// The cloud as both entry points hand it over: 64-bit offsets WITHOUT a sentinel (point i ends where point i + 1 begins,
// the last one at n_obs), SoA observations, the optional mask.
struct K15Cloud {
  uint64_t n_points, n_obs;
  const eg3d_off_t* obs_off;
  const int32_t* obs_view;
  const float* obs_xy;
  const uint8_t* keep;  // may be null: every point is kept
};

// (1) one lane per observation: words[q] = the sample of observation q, r | g << 8 | b << 16, or a K15_W_* bit (and no
//     sample) when its view id is outside the rig, its view has no image or a coordinate fails its check — each decided
//     before the value is used as an index. Uses no offset: observations of dropped points are sampled too.
void launch_k15_sample(hipStream_t st, K15Cloud c, const K15Image* images, int n_views, uint32_t* words);
// (2) one lane per point: the offsets checked, then rgb[3 i ..] = the per-channel integer mean of the point's words and
//     flags[i] (may be null) = K15_OUT_EMPTY for a kept point without observations; a dropped point gets (0, 0, 0) and 0.
//     ctr[0] |= K15_* (the K15_W_* bits of kept points' words included); ctr[1..3] += coloured points, empty points,
//     observations of kept points.
void launch_k15_mix(hipStream_t st, K15Cloud c, const uint32_t* words, uint8_t* rgb, uint8_t* flags, unsigned long long* ctr);

}  // namespace eg3d
