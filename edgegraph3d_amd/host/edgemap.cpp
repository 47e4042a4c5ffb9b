// The edge maps of the source images, their sequential statement (include/eg3d/host_edgemap.hh, K19): every rule is a
// function of csrc/eg3d_edgemap_core.h, applied here to whole images one stage after the other — the plainest order
// there is. The views of a call run on OpenMP threads; a view runs on one. Then the 1-bit PNG writer of a mask and the
// polyline graphs of many masks at once.
#include <zlib.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/eg3d/host_edgemap.hh"
#include "eg3d_edgemap_core.h"

using namespace eg3d::edgemap;

namespace {
thread_local std::string g_edgemap_err;

int refuse(int code, const char* who, const char* text) {
  g_edgemap_err = std::string(who) + ": " + text;
  return code;
}

struct ViewCounts {
  uint64_t candidates = 0, strong = 0, edges = 0;
};

// E1 - E5 and the first half of E6: the class of every pixel of one view
void classes_of_view(const uint8_t* rgb, int W, int H, const eg3d_edgemap_params& p, std::vector<uint8_t>& cls, ViewCounts& n) {
  const size_t N = (size_t)W * H;
  const bool l2 = p.l2 != 0;
  std::vector<uint8_t> a(N), b(N);
  for (size_t i = 0; i < N; i++) a[i] = (uint8_t)grey(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
  std::vector<uint16_t> hs(N);
  for (int pass = 0; pass < p.smooth_passes; pass++) {
    for (int r = 0; r < H; r++) {
      const uint8_t* row = &a[(size_t)r * W];
      for (int c = 0; c < W; c++)
        hs[(size_t)r * W + c] = (uint16_t)binom5(row[fold101(c - 2, W)], row[fold101(c - 1, W)], row[c], row[fold101(c + 1, W)], row[fold101(c + 2, W)]);
    }
    for (int r = 0; r < H; r++) {
      const uint16_t* r0 = &hs[(size_t)fold101(r - 2, H) * W];
      const uint16_t* r1 = &hs[(size_t)fold101(r - 1, H) * W];
      const uint16_t* r2 = &hs[(size_t)r * W];
      const uint16_t* r3 = &hs[(size_t)fold101(r + 1, H) * W];
      const uint16_t* r4 = &hs[(size_t)fold101(r + 2, H) * W];
      for (int c = 0; c < W; c++) b[(size_t)r * W + c] = (uint8_t)smooth_round(binom5(r0[c], r1[c], r2[c], r3[c], r4[c]));
    }
    a.swap(b);
  }
  std::vector<int16_t> gx(N), gy(N);
  std::vector<uint32_t> m(N);
  for (int r = 0; r < H; r++)
    for (int c = 0; c < W; c++) {
      int q[3][3];
      for (int dr = -1; dr <= 1; dr++)
        for (int dc = -1; dc <= 1; dc++) {
          const int rr = r + dr < 0 ? 0 : r + dr >= H ? H - 1 : r + dr, cc = c + dc < 0 ? 0 : c + dc >= W ? W - 1 : c + dc;
          q[dr + 1][dc + 1] = a[(size_t)rr * W + cc];
        }
      const size_t i = (size_t)r * W + c;
      gx[i] = (int16_t)sobel_x(q);
      gy[i] = (int16_t)sobel_y(q);
      m[i] = magnitude(gx[i], gy[i], l2);
    }
  const uint32_t lo = threshold(p.low, l2), hi = threshold(p.high, l2);
  const auto mag = [&](int r, int c) -> uint32_t { return (r < 0 || r >= H || c < 0 || c >= W) ? 0u : m[(size_t)r * W + c]; };
  cls.assign(N, kNone);
  for (int r = 0; r < H; r++)
    for (int c = 0; c < W; c++) {
      const size_t i = (size_t)r * W + c;
      const int d = nms_direction(gx[i], gy[i]);
      const bool kept = nms_keep(d, m[i], mag(r + nms_dr(d), c + nms_dc(d)), mag(r - nms_dr(d), c - nms_dc(d)));
      cls[i] = classify(kept, m[i], lo, hi);
      n.candidates += cls[i] != kNone;
      n.strong += cls[i] == kStrong;
    }
}

// E6, second half: the candidates reachable from a strong pixel over 8-neighbour steps through candidates
void mask_of_classes(std::vector<uint8_t>& cls, int W, int H, uint8_t* mask, ViewCounts& n) {
  const size_t N = (size_t)W * H;
  std::vector<uint32_t> stack;
  for (size_t i = 0; i < N; i++)
    if (cls[i] == kStrong) stack.push_back((uint32_t)i);
  while (!stack.empty()) {
    const uint32_t i = stack.back();
    stack.pop_back();
    const int r = (int)(i / (uint32_t)W), c = (int)(i % (uint32_t)W);
    for (int dr = -1; dr <= 1; dr++)
      for (int dc = -1; dc <= 1; dc++) {
        const int rr = r + dr, cc = c + dc;
        if (rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
        const size_t j = (size_t)rr * W + cc;
        if (cls[j] == kWeak) {
          cls[j] = kStrong;
          stack.push_back((uint32_t)j);
        }
      }
  }
  for (size_t i = 0; i < N; i++) {
    mask[i] = cls[i] == kStrong;
    n.edges += mask[i];
  }
}
}  // namespace

extern "C" const char* eg3d_host_edgemap_last_error(void) { return g_edgemap_err.c_str(); }

extern "C" int eg3d_host_edge_maps(int32_t n_views, const int32_t* width, const int32_t* height, const uint8_t* const* rgb,
                                   const eg3d_edgemap_params* params, uint8_t* const* masks, eg3d_edgemap_stats* stats) {
  static const char who[] = "eg3d_host_edge_maps";
  if (const char* why = refusal(n_views, width, height, rgb, params, masks, stats)) return refuse(EG3D_EDGEMAP_ERR_ARG, who, why);
  const eg3d_edgemap_params p = *params;
  std::vector<ViewCounts> counts((size_t)n_views);
  std::vector<std::vector<uint8_t>> cls((size_t)n_views);
  const auto now = [] { return std::chrono::steady_clock::now(); };
  const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<float, std::milli>(b - a).count();
  };
  int failed = 0;
  const auto t0 = now();
#pragma omp parallel for schedule(dynamic, 1)
  for (int32_t v = 0; v < n_views; v++) {
    try {
      classes_of_view(rgb[v], width[v], height[v], p, cls[(size_t)v], counts[(size_t)v]);
    } catch (const std::bad_alloc&) {
#pragma omp atomic write
      failed = 1;
    }
  }
  if (failed) return refuse(EG3D_EDGEMAP_ERR_MEMORY, who, "out of host memory");
  const auto t1 = now();
#pragma omp parallel for schedule(dynamic, 1)
  for (int32_t v = 0; v < n_views; v++) {
    try {
      mask_of_classes(cls[(size_t)v], width[v], height[v], masks[v], counts[(size_t)v]);
    } catch (const std::bad_alloc&) {
#pragma omp atomic write
      failed = 1;
    }
  }
  if (failed) return refuse(EG3D_EDGEMAP_ERR_MEMORY, who, "out of host memory");
  const auto t2 = now();
  if (stats) {
    eg3d_edgemap_stats s;
    memset(&s, 0, sizeof s);
    s.struct_size = (uint32_t)sizeof s;
    s.n_views = (uint32_t)n_views;
    for (int32_t v = 0; v < n_views; v++) {
      s.n_pixels += (uint64_t)width[v] * (uint64_t)height[v];
      s.n_candidates += counts[(size_t)v].candidates;
      s.n_strong += counts[(size_t)v].strong;
      s.n_edges += counts[(size_t)v].edges;
    }
    s.hysteresis_rounds = 1;
    s.ms_kernel = ms(t0, t1);
    s.ms_hysteresis = ms(t1, t2);
    *stats = s;
  }
  return 0;
}

// ---- the PNG writer ------------------------------------------------------------------------------------------------------
namespace {
void put_be32(std::vector<unsigned char>& o, uint32_t v) {
  for (int s = 24; s >= 0; s -= 8) o.push_back((unsigned char)(v >> s));
}
void put_chunk(std::vector<unsigned char>& o, const char* type, const unsigned char* body, size_t n) {
  put_be32(o, (uint32_t)n);
  const size_t at = o.size();
  o.insert(o.end(), type, type + 4);
  if (n) o.insert(o.end(), body, body + n);
  put_be32(o, (uint32_t)crc32(0L, &o[at], (uInt)(n + 4)));
}
}  // namespace

extern "C" int eg3d_host_png_write_mask(const char* path, const uint8_t* mask, int32_t width, int32_t height) {
  static const char who[] = "eg3d_host_png_write_mask";
  if (!path || !mask) return refuse(EG3D_EDGEMAP_ERR_ARG, who, "path or mask is NULL");
  if (!dim_ok(width) || !dim_ok(height)) return refuse(EG3D_EDGEMAP_ERR_ARG, who, "a side of the mask is < 1 or > 16384");
  try {
    // scanlines: the filter byte 0, then the pixels eight to a byte, the leftmost in the highest bit
    const size_t stride = ((size_t)width + 7) / 8;
    std::vector<unsigned char> raw((stride + 1) * (size_t)height, 0);
    for (int32_t r = 0; r < height; r++) {
      unsigned char* line = &raw[(stride + 1) * (size_t)r + 1];
      const uint8_t* src = mask + (size_t)r * width;
      for (int32_t c = 0; c < width; c++)
        if (src[c]) line[c >> 3] |= (unsigned char)(0x80 >> (c & 7));
    }
    uLongf zn = compressBound((uLong)raw.size());
    std::vector<unsigned char> z(zn);
    if (compress2(z.data(), &zn, raw.data(), (uLong)raw.size(), 6) != Z_OK) return refuse(EG3D_EDGEMAP_ERR_MEMORY, who, "deflate failed");
    std::vector<unsigned char> out = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    std::vector<unsigned char> ihdr;
    put_be32(ihdr, (uint32_t)width);
    put_be32(ihdr, (uint32_t)height);
    const unsigned char tail[5] = {1, 0, 0, 0, 0};  // 1 bit, greyscale, deflate, adaptive filtering, no interlace
    ihdr.insert(ihdr.end(), tail, tail + 5);
    put_chunk(out, "IHDR", ihdr.data(), ihdr.size());
    put_chunk(out, "IDAT", z.data(), (size_t)zn);
    put_chunk(out, "IEND", nullptr, 0);
    FILE* f = fopen(path, "wb");
    if (!f) return refuse(EG3D_EDGEMAP_ERR_FILE, who, "the file cannot be opened for writing");
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    if (fclose(f) != 0 || !ok) return refuse(EG3D_EDGEMAP_ERR_FILE, who, "the file cannot be written");
    return 0;
  } catch (const std::bad_alloc&) {
    return refuse(EG3D_EDGEMAP_ERR_MEMORY, who, "out of host memory");
  }
}

// ---- many masks to their polyline graphs -----------------------------------------------------------------------------------
extern "C" int eg3d_host_plg_build_views_from_masks(const uint8_t* const* masks, int32_t n_views, const int32_t* width,
                                                    const int32_t* height, eg3d_plg_view* out) {
  static const char who[] = "eg3d_host_plg_build_views_from_masks";
  if (n_views < 0 || (n_views && (!masks || !width || !height || !out))) return refuse(EG3D_EDGEMAP_ERR_ARG, who, "bad arguments");
  for (int32_t v = 0; v < n_views; v++)
    if (!masks[v] || width[v] < 1 || height[v] < 1) return refuse(EG3D_EDGEMAP_ERR_ARG, who, "a mask is NULL or has a side < 1");
  std::vector<int> rc((size_t)n_views, 0);
  for (int32_t v = 0; v < n_views; v++) memset(&out[v], 0, sizeof(out[v]));
#pragma omp parallel for schedule(dynamic, 1)
  for (int32_t v = 0; v < n_views; v++) rc[(size_t)v] = eg3d_plg_build_from_mask(masks[v], width[v], height[v], &out[v]);
  int bad = 0;
  for (int32_t v = 0; v < n_views && !bad; v++)
    if (rc[(size_t)v] != 0) bad = -(v + 2);
  if (bad) {
    for (int32_t v = 0; v < n_views; v++)
      if (rc[(size_t)v] == 0) eg3d_plg_view_free(&out[v]);
    return refuse(bad, who, "the build of a view failed");
  }
  return 0;
}
