// Host steps after the hot path: the order-dependent 3 px occupancy-grid dedup
// and the observation-count filter. Behaviour reproduced: filter_3d_points_close_2d_array
// (reference src/edgegraph3d/filtering/filtering_close_plgps.cpp:75-124) and the tail of
// compute_inliers / compute_ray_stats (src/edgegraph3d/filtering/outliers_filtering.cpp:14-64).
// Own design: one byte-map per view in a single allocation, greedy pass over the SoA output.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/eg3d_host.h"
#include "../../include/eg3d_host_dedup_phases.h"

// The 3 px cell grid of a rig, and the cell of an observation: -1 when it lies outside the occupancy maps (coordinates
// at or past the image border, negative, NaN, or a view id out of range). The reference indexes its arrays unchecked there
// (undefined behaviour); here such an observation never makes a point "fresh" and marks nothing — the CPU oracle adopts
// the same rule. One statement for the sequential dedup and for its phases (include/eg3d_host_dedup_phases.h).
namespace {
struct CellGrid {
  static constexpr int CELL = 3;
  int n_views, w, h;
  size_t plane;
  CellGrid(int n_views_, int width, int height)
      : n_views(n_views_), w((int)std::ceil((float)width / CELL)), h((int)std::ceil((float)height / CELL)), plane((size_t)w * h) {}
  size_t n_cells() const { return plane * (size_t)n_views; }
  int64_t cell_of(const eg3d_edgepoints* pts, uint64_t j) const {
    const int32_t v = pts->obs_view[j];
    const float fx = pts->obs_xy[2 * j] / CELL, fy = pts->obs_xy[2 * j + 1] / CELL;
    if (v < 0 || v >= n_views || !(fx > -1.0f) || !(fy > -1.0f) || !(fx < (float)w) || !(fy < (float)h)) return -1;
    const int cx = (int)fx, cy = (int)fy;
    if (cx < 0 || cy < 0 || cx >= w || cy >= h) return -1;
    return (int64_t)(plane * (size_t)v + (size_t)cy * w + cx);
  }
};
}  // namespace

extern "C" int eg3d_host_filter_close_2d(int n_views, int width, int height, const eg3d_edgepoints* pts,
                                         uint8_t* keep) {
  if (!pts || !keep || n_views <= 0) return -1;
  const CellGrid g(n_views, width, height);
  std::vector<uint8_t> occ(g.n_cells(), 0);
  for (uint64_t i = 0; i < pts->n_points; i++) {
    const uint64_t a = pts->obs_off[i], b = pts->obs_off[i + 1];
    bool fresh = false;
    for (uint64_t j = a; j < b && !fresh; j++) {
      const int64_t c = g.cell_of(pts, j);
      fresh = c >= 0 && occ[(size_t)c] == 0;
    }
    keep[i] = fresh;
    if (fresh)
      for (uint64_t j = a; j < b; j++) {
        const int64_t c = g.cell_of(pts, j);
        if (c >= 0) occ[(size_t)c] = 1;
      }
  }
  return 0;
}

// ---- the dedup in phases (include/eg3d_host_dedup_phases.h): the sequential definition of eg3d_dedup_claim / _keep /
// _merge_claims. A point that the sequential pass drops still claims here, with an index larger than the cell's owner: it
// changes no minimum, which is why the two statements agree (tests/test_dedup_phases.py holds them to each other).
static bool phases_args_ok(int n_views, int width, int height, const eg3d_edgepoints* pts, uint64_t index_base) {
  if (!pts || n_views <= 0 || width < 0 || height < 0) return false;
  if (index_base >= 0xFFFFFFFFull || pts->n_points >= 0xFFFFFFFFull - index_base) return false;
  for (uint64_t i = 0; i < pts->n_points; i++)
    if (!(pts->obs_off[i] <= pts->obs_off[i + 1] && pts->obs_off[i + 1] <= pts->n_obs)) return false;
  return true;
}
extern "C" int eg3d_host_dedup_claim(int n_views, int width, int height, const eg3d_edgepoints* pts, uint64_t index_base,
                                     uint32_t* first) {
  if (!first || !phases_args_ok(n_views, width, height, pts, index_base)) return -1;
  const CellGrid g(n_views, width, height);
  for (uint64_t i = 0; i < pts->n_points; i++) {
    const uint32_t id = (uint32_t)(index_base + i);
    for (uint64_t j = pts->obs_off[i]; j < pts->obs_off[i + 1]; j++) {
      const int64_t c = g.cell_of(pts, j);
      if (c >= 0 && id < first[c]) first[c] = id;
    }
  }
  return 0;
}
extern "C" int eg3d_host_dedup_keep(int n_views, int width, int height, const eg3d_edgepoints* pts, uint64_t index_base,
                                    const uint32_t* first, uint8_t* keep, uint64_t* n_kept) {
  if (!first || (!keep && pts && pts->n_points) || !phases_args_ok(n_views, width, height, pts, index_base)) return -1;
  const CellGrid g(n_views, width, height);
  uint64_t kept = 0;
  for (uint64_t i = 0; i < pts->n_points; i++) {
    const uint32_t id = (uint32_t)(index_base + i);
    bool mine = false;
    for (uint64_t j = pts->obs_off[i]; j < pts->obs_off[i + 1] && !mine; j++) {
      const int64_t c = g.cell_of(pts, j);
      mine = c >= 0 && first[c] == id;
    }
    keep[i] = mine;
    kept += mine;
  }
  if (n_kept) *n_kept = kept;
  return 0;
}
extern "C" int eg3d_host_dedup_merge(uint32_t* first, const uint32_t* other, uint64_t n_cells) {
  if (n_cells && (!first || !other)) return -1;
  for (uint64_t c = 0; c < n_cells; c++)
    if (other[c] < first[c]) first[c] = other[c];
  return 0;
}
extern "C" uint64_t eg3d_host_dedup_n_cells(int n_views, int width, int height) {
  return n_views > 0 && width >= 0 && height >= 0 ? (uint64_t)CellGrid(n_views, width, height).n_cells() : 0;
}

extern "C" int eg3d_host_observation_filter(int n_cameras, const uint32_t* obs_off, uint64_t n_points,
                                            uint64_t first_edgepoint, int forced_min_filter, uint8_t* inlier) {
  std::vector<uint64_t> hist((size_t)n_cameras + 1, 0);
  uint64_t count = 0;
  for (uint64_t i = 0; i < n_points; i++)
    if (inlier[i]) {
      count++;
      uint32_t k = obs_off[i + 1] - obs_off[i];
      if (k >= 1 && k <= (uint32_t)n_cameras) hist[k - 1]++;
    }
  uint64_t acc = 0;
  int median = 0;
  for (median = 0; median < n_cameras; median++) {
    acc += hist[median];
    if (acc >= count / 2) break;
  }
  int threshold = median / 2 - 1;
  if (threshold < 3) threshold = 3;  // FILTER_3VIEWS_AMOUNT
  if (forced_min_filter > -1) threshold = forced_min_filter;
  for (uint64_t i = first_edgepoint; i < n_points; i++)
    if (inlier[i] && !((int)(obs_off[i + 1] - obs_off[i]) > threshold)) inlier[i] = 0;
  return threshold;
}
