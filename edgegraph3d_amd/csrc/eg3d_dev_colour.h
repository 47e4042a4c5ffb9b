// eg3d_dev_colour.h — the per-observation colour sample of K15 (include/eg3d_colour.h), as one lane computes it.
//
// Behaviour restated from the reference's opc_getColorSubpix (io/output/output_point_cloud.cpp:65-105): a bilinear sample
// of an RGB8 image at a float position, with cv::borderInterpolate(., len, BORDER_REFLECT_101) on the four taps and
// cvRound on the result. OpenCV is not available to this project: the three OpenCV behaviours (the border rule, cvRound's
// ties-to-even, the (uchar) of an int keeping the low 8 bits) are restated from their documented semantics.
//
// Arithmetic contract: every product and sum is FP32 in the written order, no FMA (-ffp-contract=off on host and device).
// EG3D_HD functions compile for the host too: host/colour.cpp exports the closed form of the border rule so that a CPU
// test can hold it to the loop (tests/test_colour_host.py); the host STATEMENT of the sample is written on its own there.
#pragma once
#include <stdint.h>

#include "eg3d_dev_geom.h"

namespace eg3d {

#define EG3D_COLOUR_COORD_LIMIT 1e7f /* |coordinate| must stay below this: (int)px is then defined, x + 1 cannot wrap */
#define EG3D_COLOUR_MAX_OBS 32767u   /* observations of one point: the integer mean is then exactly the reference's */

// word of one observation: bits 0-7 red, 8-15 green, 16-23 blue, and in the top byte what the checks found
#define K15_W_BAD_VIEW 0x01000000u  /* a view id outside the rig */
#define K15_W_NO_IMAGE 0x02000000u  /* a view that has no image */
#define K15_W_BAD_XY 0x04000000u    /* a coordinate that is not finite, or |coordinate| >= 1e7 */
#define K15_W_BAD_MASK 0x07000000u

// NaN, +-inf and |v| >= 1e7 fail the one comparison
EG3D_HD bool colour_coord_ok(float v) { return (v < 0.f ? -v : v) < EG3D_COLOUR_COORD_LIMIT; }

// cv::borderInterpolate(p, len, BORDER_REFLECT_101) in closed form: the rule reflects about 0 and about len - 1, so it has
// the period 2 (len - 1), and inside one period the second half mirrors the first. len >= 1; any p whose p % m is defined.
EG3D_HD int colour_reflect101(int p, int len) {
  if (len == 1) return 0;
  const int m = 2 * (len - 1);
  int q = p % m;
  if (q < 0) q += m;
  return q < len ? q : m - q;
}

// One sample: rgb = the image's first byte (RGB8 interleaved, row-major, W columns, H rows), (px, py) checked by the
// caller with colour_coord_ok. Returns r | g << 8 | b << 16.
EG3D_HD uint32_t colour_sample(const uint8_t* rgb, int W, int H, float px, float py) {
  const int x = (int)px, y = (int)py;  // truncation toward zero, not floor: in (-1, 0) the weight below is negative
  const float a = px - (float)x, c = py - (float)y;
  const size_t x0 = (size_t)colour_reflect101(x, W) * 3u, x1 = (size_t)colour_reflect101(x + 1, W) * 3u;
  const uint8_t* r0 = rgb + (size_t)colour_reflect101(y, H) * (size_t)W * 3u;
  const uint8_t* r1 = rgb + (size_t)colour_reflect101(y + 1, H) * (size_t)W * 3u;
  const float na = 1.f - a, nc = 1.f - c;
  uint32_t word = 0;
  for (int ch = 0; ch < 3; ch++) {
    const float i00 = (float)r0[x0 + ch], i01 = (float)r0[x1 + ch], i10 = (float)r1[x0 + ch], i11 = (float)r1[x1 + ch];
    const float top = i00 * na + i01 * a;
    const float bot = i10 * na + i11 * a;
    const float s = top * nc + bot * c;
    // cvRound: to nearest, ties to even (the default rounding mode on both sides); (uchar) of the int: its low 8 bits
#if defined(__HIP_DEVICE_COMPILE__)
    const int q = (int)rintf(s);
#else
    const int q = (int)nearbyintf(s);
#endif
    word |= ((uint32_t)q & 0xffu) << (8 * ch);
  }
  return word;
}

}  // namespace eg3d
