// colour.cpp — eg3d_host_colour_points (include/eg3d_host_colour.h): the sequential statement of K15, point after point.
// The sample is written here on its own, with the border rule as its loop; only eg3d_host_reflect101_closed comes from the
// kernel's header, to be compared with that loop.
#include <cmath>
#include <cstdint>

#include "eg3d_dev_colour.h"
#include "eg3d_host_colour.h"

namespace {

// reflection without repeated border: p in [0, len) stays; len == 1 gives 0
int reflect101(int p, int len) {
  if (p >= 0 && p < len) return p;
  if (len == 1) return 0;
  do {
    if (p < 0)
      p = -p;
    else
      p = 2 * len - 2 - p;
  } while (p < 0 || p >= len);
  return p;
}

bool coord_ok(float v) { return std::isfinite(v) && std::fabs(v) < 1e7f; }

// one observation's three bytes; FP32 in the written order (-ffp-contract=off)
void sample(const uint8_t* img, int W, int H, float px, float py, uint8_t out[3]) {
  const int x = (int)px, y = (int)py;
  const float a = px - (float)x, c = py - (float)y;
  const int x0 = reflect101(x, W), x1 = reflect101(x + 1, W), y0 = reflect101(y, H), y1 = reflect101(y + 1, H);
  for (int ch = 0; ch < 3; ch++) {
    const float i00 = (float)img[((size_t)y0 * W + x0) * 3 + ch], i01 = (float)img[((size_t)y0 * W + x1) * 3 + ch];
    const float i10 = (float)img[((size_t)y1 * W + x0) * 3 + ch], i11 = (float)img[((size_t)y1 * W + x1) * 3 + ch];
    const float s = (i00 * (1.f - a) + i01 * a) * (1.f - c) + (i10 * (1.f - a) + i11 * a) * c;
    const int q = (int)std::lrint(s);  // to nearest, ties to even (the default rounding mode)
    out[ch] = (uint8_t)((unsigned)q & 0xffu);
  }
}

}  // namespace

extern "C" int eg3d_host_reflect101_loop(int p, int len) { return len < 1 ? -1 : reflect101(p, len); }
extern "C" int eg3d_host_reflect101_closed(int p, int len) { return len < 1 ? -1 : eg3d::colour_reflect101(p, len); }

extern "C" int eg3d_host_colour_points(int n_views, const int32_t* width, const int32_t* height, const uint8_t* const* rgb,
                                       uint64_t n_points, const uint32_t* obs_off, const int32_t* obs_view, const float* obs_xy,
                                       const uint8_t* keep, int n_threads, uint8_t* rgb_out, uint8_t* flags_out, uint64_t* counts) {
  if (n_views < 1 || !width || !height || !rgb) return -1;
  for (int v = 0; v < n_views; v++)
    if (rgb[v] && (width[v] < 1 || height[v] < 1 || width[v] > 32768 || height[v] > 32768)) return -1;
  if (counts) counts[0] = counts[1] = counts[2] = 0;
  if (!n_points) return 0;
  if (!obs_off || !rgb_out) return -1;
  for (uint64_t i = 0; i < n_points; i++)
    if (obs_off[i + 1] < obs_off[i]) return -1;
  if (obs_off[n_points] && (!obs_view || !obs_xy)) return -1;
  uint64_t n_col = 0, n_emp = 0, n_obs = 0;
  int bad = 0;
#pragma omp parallel for schedule(dynamic, 256) num_threads(n_threads > 1 ? n_threads : 1) reduction(+ : n_col, n_emp, n_obs) reduction(| : bad)
  for (int64_t i = 0; i < (int64_t)n_points; i++) {
    uint8_t* out = rgb_out + 3 * i;
    out[0] = out[1] = out[2] = 0;
    if (flags_out) flags_out[i] = 0;
    if (keep && !keep[i]) continue;
    const uint32_t a = obs_off[i], b = obs_off[i + 1], n = b - a;
    if (n > 32767u) {
      bad |= 1;
      continue;
    }
    uint32_t sum[3] = {0, 0, 0};
    bool ok = true;
    for (uint32_t k = a; k < b && ok; k++) {
      const int32_t v = obs_view[k];
      const float px = obs_xy[2 * (size_t)k], py = obs_xy[2 * (size_t)k + 1];
      if (v < 0 || v >= n_views || !rgb[v] || !coord_ok(px) || !coord_ok(py)) {
        ok = false;
        break;
      }
      uint8_t s[3];
      sample(rgb[v], width[v], height[v], px, py, s);
      sum[0] += s[0];
      sum[1] += s[1];
      sum[2] += s[2];
    }
    if (!ok) {
      bad |= 1;
      continue;
    }
    if (!n) {
      if (flags_out) flags_out[i] = 1;  // EG3D_COLOUR_FLAG_EMPTY
      n_emp++;
      continue;
    }
    out[0] = (uint8_t)(sum[0] / n);
    out[1] = (uint8_t)(sum[1] / n);
    out[2] = (uint8_t)(sum[2] / n);
    n_col++;
    n_obs += n;
  }
  if (bad) return -1;
  if (counts) {
    counts[0] = n_col;
    counts[1] = n_emp;
    counts[2] = n_obs;
  }
  return 0;
}
