// eg3d_nearest_core.h — cloud-to-cloud nearest distances (K18), the arithmetic stated once for host and device.
//
// include/eg3d/host_nearest.hpp defines the result. Here: the order-preserving code of a float for the minimum / maximum
// reduction, the cell coordinate, the key, the distance, the within rule, the better-of-two rule, the quantisation of the
// fixed-point sum, and the search of one query over a Grid — written with a lane number and a stride, so that the host
// (lane 0 of 1), a lane that owns a query (0 of 1) and the lanes of a group that share one (l of G) run the same text.
//
// GRID  origin = the component-wise minimum of the indexed points. cellcoord(x) = floor(((double)x - (double)origin) /
//   (double)cell): the difference of two floats is exact in FP64 (both are FP32 values: 24-bit significands, and the
//   division is IEEE), so the coordinate is the same number on host and device. dims[a] = cellcoord(max[a]) + 1 < 2^21.
//   key = z << 42 | y << 21 | x: x is the fastest axis, the cells xlo .. xhi of one (y, z) row are consecutive keys, and
//   because the points are stored in key order the points of those cells are ONE contiguous run: the search makes one
//   lower bound for the first key of the row's range and one for the first key after it.
//
// BOUNDS  (why nothing within reach is lost, and why the work is bounded)
//   Let r be indexed and d2(q, r) < md2. d2 >= fl(dx * dx) in FP32 — the sums add non-negative terms and rounding is
//   monotone — and fl(dx * dx) < fl(max_dist * max_dist) implies |dx| < max_dist, again because rounding is monotone:
//   |dx| >= max_dist would give fl(dx * dx) >= fl(max_dist * max_dist). dx = fl(q.x - r.x), and |q.x - r.x| < max_dist holds
//   for the real numbers as well: were the real |q.x - r.x| >= max_dist, its rounding would be >= max_dist, max_dist
//   being a float. Hence q.x - max_dist < r.x < q.x + max_dist in real numbers, and by
//   monotone rounding fl32(q.x - max_dist) <= r.x <= fl32(q.x + max_dist). cellcoord is monotone (a difference, a division
//   by a positive number and floor, each monotone, each rounding monotone), so
//   cellcoord(fl32(q.x - max_dist)) <= cellcoord(r.x) <= cellcoord(fl32(q.x + max_dist)), and r's coordinate lies inside
//   [0, dims) by construction: clamping the range to the grid loses nothing. The same holds on y and z. The comparison
//   d2 < md2 is strict, which is what makes |dx| < max_dist strict and the argument independent of how ties round.
//   With max_dist <= cell the range spans (q + max_dist) - (q - max_dist) <= 2 cell plus roundings: 3 cells per axis,
//   rarely 4 — the loops run over the range, they do not assume 3. A query far from the grid gets an empty range on
//   some axis before any conversion to an integer (the comparison is made in FP64, where +-inf is harmless).
//   Every loop is bounded: rows by the clamped ranges (<= 4 x 4 in practice, <= dims in any case), the two binary
//   searches by log2(n_cells) + 1 rounds, the run by cell_start[c1] - cell_start[c0] <= n_indexed.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/eg3d/host_nearest.hpp"
#include "eg3d_dev_geom.h"

namespace eg3d {
namespace nearest {

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kInfBits = 0x7f800000u;
constexpr int kMaxThresholds = 8;
constexpr uint32_t kAxisBits = 21;
constexpr double kMaxAxisCells = 2097152.0;  // 2^21: an axis spans fewer
constexpr uint64_t kUnindexed = ~0ull;       // the sort key of a reference point that is not indexed (no cell has it)

// one reference point in key order: its coordinates and its position in the reference array as given
struct alignas(16) Pt {
  float x, y, z;
  uint32_t j;
};

struct Grid {
  float origin[3];
  float cell;
  uint32_t dims[3];
  uint32_t n_cells;
  const uint64_t* cell_key;    // [n_cells] ascending
  const uint32_t* cell_start;  // [n_cells + 1]
  const Pt* pts;               // [n_indexed] in key order, original index ascending within a cell
};

EG3D_HD uint32_t f32_bits(float v) {
  union {
    float f;
    uint32_t u;
  } c;
  c.f = v;
  return c.u;
}
EG3D_HD float bits_f32(uint32_t u) {
  union {
    float f;
    uint32_t u;
  } c;
  c.u = u;
  return c.f;
}
EG3D_HD bool finite1(float v) { return (f32_bits(v) & 0x7f800000u) != 0x7f800000u; }
EG3D_HD bool finite3(float x, float y, float z) { return finite1(x) && finite1(y) && finite1(z); }

// a finite float as an unsigned number of the same order (-0 below +0): minimum and maximum become integer operations,
// which atomics evaluate to the same bits in any order
EG3D_HD uint32_t ordered_code(float v) {
  const uint32_t u = f32_bits(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
EG3D_HD float ordered_decode(uint32_t c) { return bits_f32((c & 0x80000000u) ? (c & 0x7fffffffu) : ~c); }

// the cell coordinate as a double: an integer value, or +-inf for an infinite x
EG3D_HD double cellcoord(float x, float origin, float cell) { return floor(((double)x - (double)origin) / (double)cell); }

EG3D_HD uint64_t cell_key(uint32_t cx, uint32_t cy, uint32_t cz) {
  return ((uint64_t)cz << (2 * kAxisBits)) | ((uint64_t)cy << kAxisBits) | (uint64_t)cx;
}
// the key of an indexed point (its coordinates lie in [0, dims) by the construction of origin and dims)
EG3D_HD uint64_t point_key(const Grid& g, float x, float y, float z) {
  return cell_key((uint32_t)cellcoord(x, g.origin[0], g.cell), (uint32_t)cellcoord(y, g.origin[1], g.cell),
                  (uint32_t)cellcoord(z, g.origin[2], g.cell));
}

EG3D_HD float dist2(float qx, float qy, float qz, float rx, float ry, float rz) {
  const float dx = qx - rx, dy = qy - ry, dz = qz - rz;
  return (dx * dx + dy * dy) + dz * dz;
}
// (d2, j) replaces (best_d2, best_j): nearer, or as near with the smaller index. best starts at (+inf, kNone) and a
// candidate is offered only when d2 < md2, so +inf never meets +inf.
EG3D_HD bool better(float d2, uint32_t j, float best_d2, uint32_t best_j) { return d2 < best_d2 || (d2 == best_d2 && j < best_j); }

EG3D_HD uint64_t quantise(float d2, float max_dist) { return (uint64_t)(sqrt((double)d2) * (4294967296.0 / (double)max_dist)); }

// the cells cellcoord(fl32(q - max_dist)) .. cellcoord(fl32(q + max_dist)) of one axis, clamped to [0, dim); false = none
EG3D_HD bool axis_range(float q, float max_dist, float origin, float cell, uint32_t dim, uint32_t* lo, uint32_t* hi) {
  const float a = q - max_dist, b = q + max_dist;
  const double tl = cellcoord(a, origin, cell), th = cellcoord(b, origin, cell);
  if (dim == 0 || th < 0.0 || tl > (double)(dim - 1)) return false;
  *lo = tl < 0.0 ? 0u : (uint32_t)tl;
  *hi = th > (double)(dim - 1) ? dim - 1 : (uint32_t)th;
  return true;
}

// the first occupied cell whose key is >= key (n_cells: none)
EG3D_HD uint32_t lower_cell(const Grid& g, uint64_t key) {
  uint32_t lo = 0, hi = g.n_cells;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (g.cell_key[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// The search of one FINITE query: candidates lane, lane + stride, ... of every row's run are offered to (*best_d2,
// *best_j), which the caller starts at (+inf, kNone). With stride > 1 the lanes' results are combined with better().
EG3D_HD void search(const Grid& g, float qx, float qy, float qz, float max_dist, float md2, uint32_t lane, uint32_t stride,
                    float* best_d2, uint32_t* best_j) {
  uint32_t x0, x1, y0, y1, z0, z1;
  if (!g.n_cells || !axis_range(qx, max_dist, g.origin[0], g.cell, g.dims[0], &x0, &x1) ||
      !axis_range(qy, max_dist, g.origin[1], g.cell, g.dims[1], &y0, &y1) ||
      !axis_range(qz, max_dist, g.origin[2], g.cell, g.dims[2], &z0, &z1))
    return;
  float bd = *best_d2;
  uint32_t bj = *best_j;
  for (uint32_t cz = z0; cz <= z1; cz++)
    for (uint32_t cy = y0; cy <= y1; cy++) {
      const uint32_t c0 = lower_cell(g, cell_key(x0, cy, cz));
      if (c0 == g.n_cells || g.cell_key[c0] > cell_key(x1, cy, cz)) continue;
      const uint32_t c1 = lower_cell(g, cell_key(x1, cy, cz) + 1);
      for (uint64_t k = (uint64_t)g.cell_start[c0] + lane, e = g.cell_start[c1]; k < e; k += stride) {
        const Pt p = g.pts[k];
        const float d2 = dist2(qx, qy, qz, p.x, p.y, p.z);
        if (d2 < md2 && better(d2, p.j, bd, bj)) {
          bd = d2;
          bj = p.j;
        }
      }
    }
  *best_d2 = bd;
  *best_j = bj;
}

// ---- the rules every entry point checks before it does anything (host code; the codes of include/eg3d/host_nearest.hpp) ----
inline int check_cell(float cell) { return (finite1(cell) && cell > 0.f) ? 0 : EG3D_NEAREST_ERR_CELL; }
inline int check_reach(float max_dist, float cell) {
  return (finite1(max_dist) && max_dist > 0.f && max_dist <= cell) ? 0 : EG3D_NEAREST_ERR_MAXDIST;
}
// t2[k] = t[k] * t[k] in FP32 for the n thresholds, +0 for the others (no d2 is below 0)
inline int check_thresholds(uint32_t n, const float* t, float max_dist, float* t2) {
  if (n > (uint32_t)kMaxThresholds) return EG3D_NEAREST_ERR_THRESHOLD;
  for (uint32_t k = 0; k < (uint32_t)kMaxThresholds; k++) t2[k] = 0.f;
  for (uint32_t k = 0; k < n; k++) {
    if (!(finite1(t[k]) && t[k] > 0.f && t[k] <= max_dist)) return EG3D_NEAREST_ERR_THRESHOLD;
    t2[k] = t[k] * t[k];
  }
  return 0;
}
// dims from the ordered minimum and maximum of the indexed points; false: 2^21 cells or more on an axis
inline bool grid_dims(const float mn[3], const float mx[3], float cell, uint32_t dims[3]) {
  for (int a = 0; a < 3; a++) {
    const double top = cellcoord(mx[a], mn[a], cell);
    if (!(top + 1.0 < kMaxAxisCells)) return false;
    dims[a] = (uint32_t)top + 1u;
  }
  return true;
}

}  // namespace nearest
}  // namespace eg3d
