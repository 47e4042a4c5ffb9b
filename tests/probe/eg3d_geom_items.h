// TEST-ONLY: one item of every table of tests/geom_cases.py through ONE call of a primitive of eg3d_dev_geom.h (and epiline of
// eg3d_dev_tri.h), written once for both compilations of those headers: the host simulation (tests/hostsim, g++) runs the items
// in a loop, the probe library (tests/probe/eg3d_probe.hip, hipcc for gfx950) one per lane. Nothing here decides anything: the
// functions unpack a row, call the primitive and pack what it returned, so that a difference between the two builds is a
// difference of the headers' code. Outputs are updated IN PLACE over whatever the caller put there (a sentinel): what a
// primitive leaves untouched stays visible.
//
// Tables (all arrays flat, row-major):
//   polylines   vtx [nv + 1][2] (one spare vertex of padding), pl_off [npl + 1] ascending, pl_start / pl_end [npl] node ids
//   walk rows   row_pl, row_seg, row_dir [n] (dir = a node id), row_f [n][8] = x y la lb lc distance min_d max_d, row_bnd [n]
//               out: status [n], seg [n], xy [n][2]
//   seg rows    in [n][8] = x1 y1 x2 y2 la lb lc thr; out: r [n], o [n][2]
//   cell rows   in [n][3] = cell x y, dims [n][4] = img_w img_h map_w map_h; out [n][4]
//   closest     row_pl, row_s0, row_s1 [n], q [n][2], boxes bb [nbb][4] with bb_off [npl + 1]; out: d [n], seg [n], xy [n][2]
//   epilines    F [n][9] double, valid [n], xy [n][2]; out: ok [n], line [n][3]
#pragma once
#include "eg3d_dev_geom.h"
#include "eg3d_dev_tri.h"

namespace eg3d_items {
using namespace eg3d;

enum : int {
  WALK_F_DISTANCE = 0,     // walk_by_distance
  WALK_F_DISTANCE_PF = 1,  // walk_by_distance_pf
  WALK_F_LINE = 2,         // walk_by_line on a global (host: plain) pointer
  WALK_F_LINE_LDS = 3,     // walk_by_line on an address_space(3) pointer: device only (eg3d_probe.hip)
  WALK_F_LINE_PF = 4,      // walk_by_line_pf
  WALK_F_HEAD1 = 5,        // walk_by_line_head<1..4> + a sequential loop of walk_seg_test + walk_resolve
  WALK_F_HEAD4 = 8,
  WALK_N_FORMS = 9
};

// the three pieces as the walk service composes them (eg3d_k3a_engine.h), without the wave: the head, then the continuation's
// segments in walking order until the first decisive test, then the resolve
template <int T>
EG3D_HD uint32_t walk_pieces(const PlRef& pl, const PlPt& p, uint32_t dir, float la, float lb, float lc, bool bounded, float min_d,
                             float max_d, PlPt& out) {
  const LineDir ld = line_dir(la, lb);
  WalkCont c;
  const uint32_t st = walk_by_line_head<T>(pl, p, dir, la, lb, lc, ld, bounded, min_d, max_d, out, c);
  if (st != WALK_UNDECIDED) return st;
  uint32_t r = 0, seg = 0;
  float hx = 0.0f, hy = 0.0f;
  for (int32_t k = 0; k < c.left; k++) {
    r = walk_seg_test(pl.v, c, k, la, lb, lc, ld, seg, hx, hy);
    if (r) break;
  }
  return walk_resolve(r, seg, hx, hy, p, bounded, min_d, max_d, out);
}

// f = the row's eight floats; `out` comes in holding the sentinel
EG3D_HD uint32_t walk_item(int form, const PlRef& pl, uint32_t seg, uint32_t dir, const float* f, bool bounded, PlPt& out) {
  PlPt p;
  p.seg = seg;
  p.x = f[0];
  p.y = f[1];
  const float la = f[2], lb = f[3], lc = f[4], distance = f[5], mn = f[6], mx = f[7];
  switch (form) {
    case WALK_F_DISTANCE: return walk_by_distance(pl, p, dir, distance, out);
    case WALK_F_DISTANCE_PF: return walk_by_distance_pf(pl, p, dir, distance, out);
    case WALK_F_LINE: return walk_by_line(pl, p, dir, la, lb, lc, bounded, mn, mx, out);
    case WALK_F_LINE_PF: return walk_by_line_pf(pl, p, dir, la, lb, lc, bounded, mn, mx, out);
    case WALK_F_HEAD1: return walk_pieces<1>(pl, p, dir, la, lb, lc, bounded, mn, mx, out);
    case WALK_F_HEAD1 + 1: return walk_pieces<2>(pl, p, dir, la, lb, lc, bounded, mn, mx, out);
    case WALK_F_HEAD1 + 2: return walk_pieces<3>(pl, p, dir, la, lb, lc, bounded, mn, mx, out);
    default: return walk_pieces<4>(pl, p, dir, la, lb, lc, bounded, mn, mx, out);
  }
}

enum : int {
  SEG_M_HIT = 0,      // seg_line_hit: r = found, o = the hit (untouched without one)
  SEG_M_GUARDED = 1,  // seg_line_hit_guarded: r = its two bits, o = the hit
  SEG_M_PLDIST = 2,   // point_line_dist of (x1, y1): o[0]
  SEG_M_COS_GT = 3,   // r = bit 0 seg_line_cos_gt, bit 1 seg_line_cos(...) > thr; o[0] = seg_line_cos
  SEG_N_MODES = 4
};
EG3D_HD void seg_item(int mode, const float* q, uint32_t& r, float* o) {
  if (mode == SEG_M_HIT) {
    r = seg_line_hit(q[0], q[1], q[2], q[3], q[4], q[5], q[6], o[0], o[1]) ? 1u : 0u;
  } else if (mode == SEG_M_GUARDED) {
    const LineDir ld = line_dir(q[4], q[5]);
    r = seg_line_hit_guarded(q[0], q[1], q[2], q[3], q[4], q[5], q[6], ld, o[0], o[1]);
  } else if (mode == SEG_M_PLDIST) {
    r = 0;
    o[0] = point_line_dist(q[0], q[1], q[4], q[5], q[6]);
  } else {
    const LineDir ld = line_dir(q[4], q[5]);
    const float cs = seg_line_cos(q[0], q[1], q[2], q[3], q[4], q[5]);
    r = (seg_line_cos_gt(q[0], q[1], q[2], q[3], ld, q[7]) ? 1u : 0u) | (cs > q[7] ? 2u : 0u);
    o[0] = cs;
  }
}

enum : int { CELL_M_OF = 0, CELL_M_WINDOW = 1, CELL_N_MODES = 2 };
// cell_of: col, row, bx, by; cell_window: c0, c1, r0, r1
EG3D_HD void cell_item(int mode, const float* q, const int32_t* dims, int32_t* o) {
  if (mode == CELL_M_OF) {
    const CellCoord c = cell_of(q[0], q[1], q[2]);
    o[0] = c.col;
    o[1] = c.row;
    o[2] = c.bx ? 1 : 0;
    o[3] = c.by ? 1 : 0;
  } else {
    const CellWindow w = cell_window(q[0], dims[0], dims[1], dims[2], dims[3], q[1], q[2]);
    o[0] = w.c0;
    o[1] = w.c1;
    o[2] = w.r0;
    o[3] = w.r1;
  }
}

enum : int { CLOSEST_M_WHOLE = 0, CLOSEST_M_RANGE = 1, CLOSEST_M_PRUNED = 2, CLOSEST_N_MODES = 3 };
// pl.bb = the polyline's block boxes for CLOSEST_M_PRUNED (nullptr otherwise)
EG3D_HD float closest_item(int mode, const PlRef& pl, float px, float py, uint32_t s0, uint32_t s1, PlPt& out) {
  if (mode == CLOSEST_M_WHOLE) return polyline_closest(pl, px, py, out);
  if (mode == CLOSEST_M_RANGE) return polyline_closest_range(pl, px, py, s0, s1, out);
  return polyline_closest_pruned(pl, px, py, s0, s1, out);
}

// one pair per row: the row's matrix and validity byte are "view pair (0, 0) of one view"
EG3D_HD int32_t epiline_item(const double* F9, const uint8_t* valid, float x, float y, float* line) {
  return epiline(F9, valid, 1, 0, 0, x, y, line[0], line[1], line[2]) ? 1 : 0;
}

// ---- what every caller checks BEFORE any item runs (the tables' input contract): returns false for a broken table
inline bool finite_f(float v) { return v - v == 0.0f; }
inline bool polylines_ok(const float* vtx, uint64_t nv, const uint32_t* pl_off, uint32_t npl) {
  if (!vtx || !pl_off || npl < 1 || pl_off[0] != 0) return false;
  for (uint32_t p = 0; p < npl; p++)
    if (pl_off[p + 1] < pl_off[p] + 2 || pl_off[p + 1] > nv) return false;  // ascending, n >= 2, inside the vertex array
  if (pl_off[npl] != nv) return false;
  for (uint64_t i = 0; i < 2 * (nv + 1); i++)  // (the spare vertex too)
    if (!finite_f(vtx[i])) return false;
  return true;
}
inline bool walk_rows_ok(const uint32_t* pl_off, uint32_t npl, uint64_t n, const uint32_t* row_pl, const uint32_t* row_seg) {
  for (uint64_t i = 0; i < n; i++) {
    if (row_pl[i] >= npl) return false;
    const uint32_t nvert = pl_off[row_pl[i] + 1] - pl_off[row_pl[i]];
    if (row_seg[i] > nvert - 2) return false;
  }
  return true;
}
inline bool closest_rows_ok(const uint32_t* pl_off, uint32_t npl, const uint32_t* bb_off, uint64_t nbb, uint64_t n,
                            const uint32_t* row_pl, const uint32_t* row_s0, const uint32_t* row_s1) {
  for (uint32_t p = 0; p < npl; p++) {
    const uint32_t nseg = pl_off[p + 1] - pl_off[p] - 1;
    if (bb_off[p + 1] < bb_off[p] || bb_off[p + 1] - bb_off[p] != (nseg + EG3D_BB_SEGS - 1) / EG3D_BB_SEGS || bb_off[p + 1] > nbb)
      return false;
  }
  for (uint64_t i = 0; i < n; i++) {
    if (row_pl[i] >= npl) return false;
    const uint32_t nvert = pl_off[row_pl[i] + 1] - pl_off[row_pl[i]];
    if (row_s1[i] > nvert - 1 || row_s0[i] > nvert - 1) return false;
  }
  return true;
}

}  // namespace eg3d_items
