// eg3d_matched_core.h — "is this point of a 2-D polyline already matched?", stated once for host and device.
//
// The reference's PLGMatchesManager keeps, per (view, polyline), a set of matched intervals ordered by the segment index
// of their start (plg_matches_manager.hpp:60-65: one interval per start segment). Two functions of it decide what the
// pipelines 1-2 extractor skips (polyline_matching.cpp:65,175):
//
//   interval_contains_plp   polyline_graph_2d.cpp:269-293
//   is_matched              plg_matches_manager.cpp:54-85
//
// Both are restated here on ONE polyline's row of the interval CSR (eg3d_graph3d / eg3d_device_graph3d: iv_off over the
// scene's global polyline index, start segments strictly ascending within a row). Behaviour, not code; what the reference
// does there and what therefore decides the output is kept, including what looks like an oversight:
//
//   M1  `pli.start.segment_index - 1` is unsigned 64-bit arithmetic: for an interval that starts on segment 0 the first
//       test reads `plp.segment_index < 2^64 - 1`, which holds for every point — such an interval contains nothing.
//   M2  the "strictly inside" test (:272) compares the point's segment with the START segment on both sides and can never
//       be true: a point on a segment strictly between an interval's start and end segment is not contained by this test.
//   M3  is_matched looks at the interval that starts on the point's own segment; when that one does not contain the point
//       (or there is none) it looks at the interval before it, and at that one only when its END segment is <= the
//       point's segment. Together with M2: a point in the middle of a long interval is "not matched".
//   M4  when every interval of the row starts after the point's segment the reference decrements begin() of its std::set,
//       which is undefined. DEFINED HERE as "not matched".
//
// The walk of the extractor jumps to the end of the containing interval and goes on from there; the reference loops for
// ever when that lands at or behind the point it came from (an interval whose end lies before its start, which the
// quirks above let "contain" a point). walk_progresses is the test every user of this header applies to refuse that.
#pragma once
#include "eg3d_dev_geom.h"

namespace eg3d {

// matched_polyline_intervals as the CSR of eg3d_graph3d (host or device pointers)
struct IvTable {
  const uint64_t* off;  // [n_scene_polylines + 1]
  const uint32_t* start_seg;
  const float* start_xy;  // [..][2]
  const uint32_t* end_seg;
  const float* end_xy;
};
// one polyline's row of it
struct IvRow {
  const uint32_t* start_seg;
  const float* start_xy;
  const uint32_t* end_seg;
  const float* end_xy;
  uint32_t n;
};
EG3D_HD IvRow iv_row_at(const IvTable& t, uint64_t r0, uint64_t r1) {
  IvRow r;
  r.start_seg = t.start_seg + r0;
  r.start_xy = t.start_xy + 2 * r0;
  r.end_seg = t.end_seg + r0;
  r.end_xy = t.end_xy + 2 * r0;
  r.n = (uint32_t)(r1 - r0);
  return r;
}
EG3D_HD IvRow iv_row(const IvTable& t, uint32_t g) { return iv_row_at(t, t.off[g], t.off[g + 1]); }

// is_ordered_2dlinepoints (geometric_utilities.cpp:1375-1377), the form of `ordered` in host/replay.cpp and K8
EG3D_HD bool ordered_2dlinepoints(float ax, float ay, float bx, float by, float cx, float cy) {
  return (bx - ax) * (cx - bx) > 0 || (by - ay) * (cy - by) > 0 || ((ax == bx && ay == by) || (bx == cx && by == cy));
}

// polyline::interval_contains_plp for interval i of the row; v = the polyline's vertices. Preconditions (checked by
// check_interval_row and by the producers of p): both segment indices of the interval and p.seg are < vertex count - 1.
EG3D_HD bool interval_contains_plp(const IvRow& r, uint32_t i, const f2* v, const PlPt& p) {
  const uint64_t s = r.start_seg[i], e = r.end_seg[i], ps = p.seg;
  const float sx = r.start_xy[2 * i], sy = r.start_xy[2 * i + 1];
  const float ex = r.end_xy[2 * i], ey = r.end_xy[2 * i + 1];
  if (ps < s - 1 /* M1: wraps for s == 0 */ || ps > e + 1) return false;
  // (M2: `ps > s && ps < s` — never)
  if (ps == s) {
    if (!ordered_2dlinepoints(v[s].x, v[s].y, sx, sy, p.x, p.y)) return false;
    return e == s ? ordered_2dlinepoints(sx, sy, p.x, p.y, ex, ey) : true;
  }
  if (ps == e) return ordered_2dlinepoints(v[e].x, v[e].y, p.x, p.y, ex, ey);
  if (ps == e + 1 && v[ps].x == p.x && v[ps].y == p.y && ex == v[ps].x && ey == v[ps].y) return true;  // coincides with end
  if (ps == s - 1 && v[ps + 1].x == p.x && v[ps + 1].y == p.y && sx == v[ps + 1].x && sy == v[ps + 1].y)
    return true;  // coincides with start
  return false;
}

// PLGMatchesManager::is_matched on one row: the index (within the row) of the interval that holds p, or -1.
EG3D_HD int32_t is_matched(const IvRow& r, const f2* v, const PlPt& p) {
  if (!r.n) return -1;
  uint32_t lo = 0, hi = r.n;  // lower_bound: first interval with start segment >= p.seg
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (r.start_seg[mid] < p.seg)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo < r.n && r.start_seg[lo] == p.seg) {
    if (interval_contains_plp(r, lo, v, p)) return (int32_t)lo;
    if (lo == 0) return -1;  // reached_begin
  } else if (lo == 0) {
    return -1;  // M4
  }
  const uint32_t i = lo - 1;  // M3: the interval before, only when it ends on or before the point's segment
  if (r.end_seg[i] <= p.seg && interval_contains_plp(r, i, v, p)) return (int32_t)i;
  return -1;
}

// `next` lies strictly further along the polyline than `last`: (segment, then distance from that segment's first vertex —
// compared squared, dist2: no rounding of a square root can make two different distances equal)
EG3D_HD bool walk_progresses(const f2* v, const PlPt& last, const PlPt& next) {
  if (next.seg != last.seg) return next.seg > last.seg;
  return dist2(v[next.seg].x, v[next.seg].y, next.x, next.y) > dist2(v[last.seg].x, v[last.seg].y, last.x, last.y);
}

// What is checked of row g before anything indexes with it (one lane per row on the device, a loop on the host):
// offsets ascending and inside [0, total]; both segment indices inside the polyline (n_vtx vertices: segments
// 0 .. n_vtx - 2), so no interval on a polyline with fewer than two vertices; start segments strictly ascending.
EG3D_HD bool check_interval_row(const IvTable& t, uint64_t total, uint32_t g, uint32_t n_vtx) {
  const uint64_t r0 = t.off[g], r1 = t.off[g + 1];
  if (r0 > r1 || r1 > total) return false;
  if (r1 > r0 && n_vtx < 2) return false;
  for (uint64_t k = r0; k < r1; k++) {
    if (t.start_seg[k] >= n_vtx - 1 || t.end_seg[k] >= n_vtx - 1) return false;
    if (k > r0 && t.start_seg[k] <= t.start_seg[k - 1]) return false;
  }
  return true;
}

}  // namespace eg3d
