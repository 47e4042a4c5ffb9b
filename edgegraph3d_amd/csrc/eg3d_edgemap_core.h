// eg3d_edgemap_core.h — the edge maps of the source images (K19), the per-pixel rules stated once for host and device.
//
// include/eg3d/host_edgemap.hh defines the result (E1 - E7). Here: the grey value, the reflect-101 fold, the 5-tap binomial
// and the rounding of a smoothing pass, the Sobel pair, the magnitude and the thresholds in their two forms, the
// direction of the non-maximum suppression, its keep rule and the class of a pixel. Every value is an integer; nothing
// here depends on the order of evaluation, so the host statement (host/edgemap.cpp), the kernels (eg3d_k19_edgemap.hip)
// and a restatement in another language agree bit for bit.
//
// RANGES  A grey value and a smoothed value are 0 .. 255: 4899 + 9617 + 1868 = 16384, so E1 maps (255, 255, 255) to
//   (16384 * 255 + 8192) >> 14 = 255, and a pass maps a constant 255 to (255 * 256 + 128) >> 8 = 255. The sum of one
//   direction of a pass is at most 255 * 16 = 4080 (16 bits), of both 65 280. |gx|, |gy| <= 4 * 255 = 1020; the L1
//   magnitude is at most 2040, the squared one at most 2 080 800; low^2 and high^2 are at most 65535^2 < 2^32. Everything
//   but the direction test of E5 fits 32 bits; that test is evaluated in 64.
#pragma once
#include <stdint.h>

#include "../../include/eg3d/host_edgemap.hh"
#include "eg3d_dev_geom.h"

namespace eg3d {
namespace edgemap {

constexpr int kMaxDim = EG3D_EDGEMAP_MAX_DIM;                     // a side of an image: 1 .. kMaxDim
constexpr int kMaxSmoothPasses = EG3D_EDGEMAP_MAX_SMOOTH_PASSES;  // smooth_passes: 0 .. kMaxSmoothPasses
constexpr int kMaxThreshold = EG3D_EDGEMAP_MAX_THRESHOLD;         // 0 <= low <= high <= kMaxThreshold
static_assert(kMaxDim <= 32768 && kMaxThreshold <= 65535, "a pixel index fits 32 bits; a squared bound fits 32 bits");
constexpr int kSmoothHalo = 2;        // pixels a smoothing pass reads beyond its output, per side
// the class of a pixel after E6's first half; hysteresis turns the weak candidates of a component with a strong one strong
enum : uint8_t { kNone = 0, kWeak = 1, kStrong = 2 };

// E1
EG3D_HD int grey(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14; }

// E2: the index an out-of-image index folds to (reflect-101), defined for every i and every n >= 1
EG3D_HD int fold101(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i = (i < 0 ? -i : i) % p;
  return i >= n ? p - i : i;
}
// E2: one direction of a pass, and the rounding after both
EG3D_HD int binom5(int a, int b, int c, int d, int e) { return a + 4 * b + 6 * c + 4 * d + e; }
EG3D_HD int smooth_round(int sum) { return (sum + 128) >> 8; }

// E3: p[r][c] is the 3 x 3 neighbourhood (borders replicated by the caller), r down, c right
EG3D_HD int sobel_x(const int p[3][3]) { return (p[0][2] + 2 * p[1][2] + p[2][2]) - (p[0][0] + 2 * p[1][0] + p[2][0]); }
EG3D_HD int sobel_y(const int p[3][3]) { return (p[2][0] + 2 * p[2][1] + p[2][2]) - (p[0][0] + 2 * p[0][1] + p[0][2]); }

// E4
EG3D_HD uint32_t magnitude(int gx, int gy, bool l2) {
  const uint32_t ax = (uint32_t)(gx < 0 ? -gx : gx), ay = (uint32_t)(gy < 0 ? -gy : gy);
  return l2 ? ax * ax + ay * ay : ax + ay;
}
EG3D_HD uint32_t threshold(int t, bool l2) { return l2 ? (uint32_t)t * (uint32_t)t : (uint32_t)t; }

// E5: which two neighbours a pixel is compared with. 0: left and right; 1: up and down; 2: the diagonal with s = 1
// (up-left and down-right); 3: the diagonal with s = -1 (up-right and down-left).
EG3D_HD int nms_direction(int gx, int gy) {
  const int64_t x = gx < 0 ? -gx : gx, y = (int64_t)(gy < 0 ? -gy : gy) << 15;
  const int64_t t22 = x * 13573, t67 = t22 + (x << 16);
  if (y < t22) return 0;
  if (y > t67) return 1;
  return ((gx ^ gy) < 0) ? 3 : 2;
}
// first / second: the magnitudes of the direction's two neighbours in E5's order (0 outside the image)
EG3D_HD bool nms_keep(int direction, uint32_t m, uint32_t first, uint32_t second) {
  return direction < 2 ? (m > first && m >= second) : (m > first && m > second);
}
// the column offset of the direction's FIRST neighbour (its row offset is 0 for direction 0, -1 otherwise); the second
// neighbour lies opposite
EG3D_HD int nms_dc(int direction) { return direction == 0 ? -1 : direction == 1 ? 0 : direction == 2 ? -1 : 1; }
EG3D_HD int nms_dr(int direction) { return direction == 0 ? 0 : -1; }

// E6, first half
EG3D_HD uint8_t classify(bool kept, uint32_t m, uint32_t low, uint32_t high) {
  return (kept && m > low) ? (m > high ? kStrong : kWeak) : kNone;
}

// E7: the parameters
EG3D_HD bool params_ok(int low, int high, int smooth_passes, int l2) {
  return 0 <= low && low <= high && high <= kMaxThreshold && 0 <= smooth_passes && smooth_passes <= kMaxSmoothPasses && (l2 == 0 || l2 == 1);
}
EG3D_HD bool dim_ok(int n) { return n >= 1 && n <= kMaxDim; }

// E7: the rule a call breaks (the first in this order), or nullptr. Host only; both libraries refuse with this text.
inline const char* refusal(int32_t n_views, const int32_t* width, const int32_t* height, const uint8_t* const* rgb,
                           const eg3d_edgemap_params* params, uint8_t* const* masks, const eg3d_edgemap_stats* stats) {
  if (stats && stats->struct_size < sizeof(eg3d_edgemap_stats)) return "stats->struct_size is smaller than sizeof(eg3d_edgemap_stats)";
  if (!params) return "params is NULL";
  if (params->struct_size < sizeof(eg3d_edgemap_params)) return "params->struct_size is smaller than sizeof(eg3d_edgemap_params)";
  if (n_views <= 0) return "n_views <= 0";
  if (!width || !height || !rgb || !masks) return "width, height, rgb or masks is NULL";
  if (!params_ok(params->low, params->high, params->smooth_passes, params->l2))
    return "parameters out of range (0 <= low <= high <= 65535, smooth_passes 0 .. 4, l2 0 or 1)";
  for (int32_t v = 0; v < n_views; v++) {
    if (!dim_ok(width[v]) || !dim_ok(height[v])) return "a side of an image is < 1 or > 16384";
    if (!rgb[v] || !masks[v]) return "an image or a mask of a view is NULL";
  }
  return nullptr;
}

}  // namespace edgemap
}  // namespace eg3d
