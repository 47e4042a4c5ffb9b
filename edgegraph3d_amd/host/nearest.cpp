// nearest.cpp — eg3d_host_cloud_nearest, eg3d_host_cloud_index_stats (include/eg3d/host_nearest.hpp): the sequential
// statement of K18. Its own grid — a std::sort of (key, original index) pairs where the device uses a radix sort — and
// the search, the within rule and the quantisation of csrc/eg3d_nearest_core.h. The queries are independent of each
// other and the figures are taken from the finished d2 array in index order, so the per-query loop may run on several
// threads (OpenMP, OMP_NUM_THREADS) without changing a bit.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "eg3d_nearest_core.h"

using namespace eg3d::nearest;

namespace eg3d {
namespace nearest {
thread_local std::string g_host_err;  // (ply_read.cpp writes it too)
}
}  // namespace eg3d

extern "C" const char* eg3d_host_nearest_last_error(void) { return g_host_err.c_str(); }

namespace {

int refuse(int code, const std::string& text) {
  g_host_err = text;
  return code;
}

struct HostGrid {
  Grid g{};
  std::vector<uint64_t> cell_key;
  std::vector<uint32_t> cell_start;
  std::vector<Pt> pts;
  uint64_t n_dropped = 0, n_nonfinite = 0, max_cell = 0;
};

// 0, or the code of the extent refusal
int build_grid(const float* X, uint64_t n, const uint8_t* keep, float cell, HostGrid* h) {
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0, 0, 0};
  uint64_t n_indexed = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (keep && !keep[i]) {
      h->n_dropped++;
      continue;
    }
    if (!finite3(X[3 * i], X[3 * i + 1], X[3 * i + 2])) {
      h->n_nonfinite++;
      continue;
    }
    n_indexed++;
    for (int a = 0; a < 3; a++) {
      const uint32_t c = ordered_code(X[3 * i + a]);
      lo[a] = std::min(lo[a], c);
      hi[a] = std::max(hi[a], c);
    }
  }
  Grid& g = h->g;
  g.cell = cell;
  if (!n_indexed) {
    h->cell_start.assign(1, 0u);
    g.cell_key = h->cell_key.data();
    g.cell_start = h->cell_start.data();
    g.pts = h->pts.data();
    return 0;
  }
  float mn[3], mx[3];
  for (int a = 0; a < 3; a++) {
    mn[a] = g.origin[a] = ordered_decode(lo[a]);
    mx[a] = ordered_decode(hi[a]);
  }
  if (!grid_dims(mn, mx, cell, g.dims)) return EG3D_NEAREST_ERR_EXTENT;
  std::vector<std::pair<uint64_t, uint32_t>> order;
  order.reserve(n_indexed);
  for (uint64_t i = 0; i < n; i++)
    if ((!keep || keep[i]) && finite3(X[3 * i], X[3 * i + 1], X[3 * i + 2]))
      order.emplace_back(point_key(g, X[3 * i], X[3 * i + 1], X[3 * i + 2]), (uint32_t)i);
  std::sort(order.begin(), order.end());  // (key, then original index)
  h->pts.resize(n_indexed);
  for (uint64_t k = 0; k < n_indexed; k++) {
    const uint32_t j = order[k].second;
    h->pts[k] = Pt{X[3 * (uint64_t)j], X[3 * (uint64_t)j + 1], X[3 * (uint64_t)j + 2], j};
    if (k == 0 || order[k].first != order[k - 1].first) {
      h->cell_key.push_back(order[k].first);
      h->cell_start.push_back((uint32_t)k);
    }
  }
  h->cell_start.push_back((uint32_t)n_indexed);
  g.n_cells = (uint32_t)h->cell_key.size();
  for (uint32_t c = 0; c < g.n_cells; c++) h->max_cell = std::max<uint64_t>(h->max_cell, h->cell_start[c + 1] - h->cell_start[c]);
  g.cell_key = h->cell_key.data();
  g.cell_start = h->cell_start.data();
  g.pts = h->pts.data();
  return 0;
}

int check_reference(const char* who, const float* ref_X, uint64_t n_ref, float cell) {
  if (n_ref && !ref_X) return refuse(EG3D_NEAREST_ERR_ARG, std::string(who) + ": ref_X is NULL");
  if (check_cell(cell)) return refuse(EG3D_NEAREST_ERR_CELL, std::string(who) + ": cell must be finite and > 0");
  if (n_ref >= (1ull << 32)) return refuse(EG3D_NEAREST_ERR_CAPACITY, std::string(who) + ": 2^32 reference points or more");
  return 0;
}

}  // namespace

extern "C" int eg3d_host_cloud_index_stats(const float* ref_X, uint64_t n_ref, const uint8_t* ref_keep, float cell,
                                           eg3d_cloud_index_stats* stats) {
  const char* who = "eg3d_host_cloud_index_stats";
  if (!stats || stats->struct_size < sizeof(eg3d_cloud_index_stats))
    return refuse(EG3D_NEAREST_ERR_ARG, std::string(who) + ": stats is NULL or its struct_size is smaller than this library's");
  if (int rc = check_reference(who, ref_X, n_ref, cell)) return rc;
  const auto w0 = std::chrono::steady_clock::now();
  HostGrid h;
  if (int rc = build_grid(ref_X, n_ref, ref_keep, cell, &h)) return refuse(rc, std::string(who) + ": 2^21 cells or more on an axis");
  eg3d_cloud_index_stats s{};
  s.struct_size = (uint32_t)sizeof(s);
  s.n_points = n_ref;
  s.n_dropped = h.n_dropped;
  s.n_nonfinite = h.n_nonfinite;
  s.n_indexed = h.pts.size();
  s.n_cells = h.g.n_cells;
  s.max_cell_points = h.max_cell;
  for (int a = 0; a < 3; a++) s.origin[a] = h.g.origin[a], s.dims[a] = h.g.dims[a];
  s.cell = cell;
  s.ms_build = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
  *stats = s;
  return 0;
}

extern "C" int eg3d_host_cloud_nearest(const float* ref_X, uint64_t n_ref, const uint8_t* ref_keep, const float* X, uint64_t n,
                                       const uint8_t* keep, float cell, float max_dist, float* d2, uint32_t* nn,
                                       eg3d_nearest_stats* stats) {
  const char* who = "eg3d_host_cloud_nearest";
  if (stats && stats->struct_size < sizeof(eg3d_nearest_stats))
    return refuse(EG3D_NEAREST_ERR_ARG, std::string(who) + ": stats->struct_size is smaller than this library's eg3d_nearest_stats");
  if (int rc = check_reference(who, ref_X, n_ref, cell)) return rc;
  if (n && !X) return refuse(EG3D_NEAREST_ERR_ARG, std::string(who) + ": X is NULL");
  if (check_reach(max_dist, cell)) return refuse(EG3D_NEAREST_ERR_MAXDIST, std::string(who) + ": max_dist must be finite, > 0 and <= cell");
  float t2[kMaxThresholds];
  if (check_thresholds(stats ? stats->n_thresholds : 0, stats ? stats->thresholds : nullptr, max_dist, t2))
    return refuse(EG3D_NEAREST_ERR_THRESHOLD, std::string(who) + ": at most 8 thresholds, each finite and in (0, max_dist]");
  if (n >= (1ull << 32)) return refuse(EG3D_NEAREST_ERR_CAPACITY, std::string(who) + ": 2^32 queries or more");
  const auto w0 = std::chrono::steady_clock::now();
  HostGrid h;
  if (int rc = build_grid(ref_X, n_ref, ref_keep, cell, &h)) return refuse(rc, std::string(who) + ": 2^21 cells or more on an axis");
  std::vector<float> d2_own;
  if (!d2) {
    d2_own.resize(n);
    d2 = d2_own.data();
  }
  const float md2 = max_dist * max_dist;
  const Grid g = h.g;
#pragma omp parallel for schedule(dynamic, 4096)
  for (int64_t i = 0; i < (int64_t)n; i++) {
    float bd = bits_f32(kInfBits);
    uint32_t bj = kNone;
    const float qx = X[3 * i], qy = X[3 * i + 1], qz = X[3 * i + 2];
    if ((!keep || keep[i]) && finite3(qx, qy, qz)) search(g, qx, qy, qz, max_dist, md2, 0u, 1u, &bd, &bj);
    d2[i] = bd;
    if (nn) nn[i] = bj;
  }
  if (stats) {
    eg3d_nearest_stats s = *stats;  // (the thresholds stay)
    s.struct_size = (uint32_t)sizeof(s);
    s.n_queries = n;
    s.n_dropped = s.n_nonfinite = s.n_within = s.sum_q32 = 0;
    for (int k = 0; k < kMaxThresholds; k++) s.n_below[k] = 0;
    std::vector<uint32_t> bits(n);
    uint32_t lo = kInfBits, hi = 0;
    for (uint64_t i = 0; i < n; i++) {
      bits[i] = f32_bits(d2[i]);
      if (keep && !keep[i])
        s.n_dropped++;
      else if (!finite3(X[3 * i], X[3 * i + 1], X[3 * i + 2]))
        s.n_nonfinite++;
      if (bits[i] == kInfBits) continue;
      s.n_within++;
      lo = std::min(lo, bits[i]);
      hi = std::max(hi, bits[i]);
      s.sum_q32 += quantise(d2[i], max_dist);
      for (uint32_t k = 0; k < s.n_thresholds; k++) s.n_below[k] += d2[i] < t2[k] ? 1u : 0u;
    }
    uint32_t med = kInfBits;
    if (s.n_within) {
      std::nth_element(bits.begin(), bits.begin() + (s.n_within - 1) / 2, bits.end());  // (unsigned order: +inf last)
      med = bits[(s.n_within - 1) / 2];
    }
    s.min_d2 = bits_f32(s.n_within ? lo : kInfBits);
    s.max_d2 = bits_f32(s.n_within ? hi : kInfBits);
    s.median_d2 = bits_f32(med);
    s.ms_kernel = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
    s.ms_copy = 0.f;
    *stats = s;
  }
  return 0;
}
