// eg3d_edges_core.h — the 3-D edge model of the matched graph (K17), stated once for host and device.
//
// Input: the geometric half of a graph3d (eg3d_graph3d / eg3d_device_graph3d): n_nodes, node_X, n_polylines, pl_start,
// pl_end, conn_off, conn_pl. Every polyline of that graph is one direct connection between two nodes. Three steps:
//
// TRACE  (the rules; they do not depend on the order in which the graph is traversed)
//   loop         a polyline with pl_start == pl_end: never in a chain, not counted in a degree, counted in the stats
//   degree       of a node: the non-loop polylines of its conn row. 2 = pass-through, any other degree >= 1 = terminal,
//                0 = in no chain
//   chain        a maximal sequence of non-loop polylines in which consecutive ones meet in a pass-through node: OPEN when
//                it ends in terminals (which may be one and the same node), a RING when every node on it is pass-through
//   numbering    by the smallest polyline id of the chain, ascending
//   orientation  open: from the end whose end polyline has the smaller id; one polyline: pl_start -> pl_end.
//                ring: from its smallest node id along the smaller of that node's two polyline ids, the start node
//                repeated as the last vertex
//   A HALF-EDGE is (polyline, side): h = 2 p + side; side 0 runs pl_start -> pl_end, side 1 the other way. The successor
//   of a half-edge is the half-edge that leaves its far node along that node's other polyline when the far node is
//   pass-through, none otherwise. The host walks the successors; the kernels rank them by pointer jumping.
//
// SIMPLIFY  simplify_polyline of the reference (plgs/polyline_graph_3d.cpp:147-250) on a chain's vertex list:
//   linearizable_polyline, find_max_se, find_min_eb, find_compatible_se_eb as written there — the strict `>` of the test,
//   the order in which candidates are tried. distance_point_line_sq is |cross(d, a - p)|^2 / |d|^2 with d = b - a
//   (geometric_utilities.cpp:1003-1005, datatypes.cpp:60-69) in FP32, no FMA, in glm's evaluation order:
//   cross(x, y) = (x.y y.z - y.y x.z, x.z y.x - y.z x.x, x.x y.y - y.x x.y), dot = (x x + y y) + z z. PINNED against the
//   reference's vendored glm (tests/test_edges_glm_pin.py). maxsq = max_dist * max_dist in FP32.
//   The test is handed in as a functor, so that the host evaluates it point after point and a wavefront 64 points at a
//   time: "any distance > maxsq" is a predicate, the result is the same.
//   DEVIATION (E1). When a chain's first and last vertex are the same node, the line through them has direction 0, every
//   distance is 0 / 0 = NaN and `NaN > maxsq` is false: the reference's rule calls the whole chain linear and collapses it
//   to two equal points. Such a chain is simplified WITHOUT its last vertex, which is appended again afterwards.
//   Kept vertices go to a region of the chain's own length: the front list from the left, the end list from the right,
//   so the kept vertices in order are region[0, nf) and region[n - nb, n).
//
// LENGTH  update_length (:57-61): the FP32 sum, in vertex order, of compute_3d_distance — the squared distance through
//   pow(float, 2) in double, summed in double, rounded once, then the FP32 square root (as sqdist / dist of
//   host/plg_build.cpp state it for 2-D, Q5).
//
// BOUNDS  every loop below is bounded by the chain's vertex count n: `start` advances in every outer round of
//   simplify_indices (se >= start + 1: in round k of find_compatible_se_eb se <= end - k and eb >= min(start + k, end - 1),
//   so eb >= se after at most (end - start + 1) / 2 rounds, long before max_se <= start), and the rounds are counted as well.
#pragma once
#include <stdint.h>

#include "eg3d_dev_geom.h"

namespace eg3d {
namespace edges {

constexpr uint32_t kNone = 0xFFFFFFFFu;
// node and polyline counts stay below this: half-edge ids and the ranks of the pointer jumping are 32-bit
constexpr uint64_t kMaxCount = 1ull << 30;

// ---- half-edges --------------------------------------------------------------------------------------------------------
EG3D_HD uint32_t he_polyline(uint32_t h) { return h >> 1; }
EG3D_HD uint32_t he_from(uint32_t h, const uint32_t* pl_start, const uint32_t* pl_end) { return (h & 1u) ? pl_end[h >> 1] : pl_start[h >> 1]; }
EG3D_HD uint32_t he_far(uint32_t h, const uint32_t* pl_start, const uint32_t* pl_end) { return (h & 1u) ? pl_start[h >> 1] : pl_end[h >> 1]; }

// the non-loop polylines of node v's row
EG3D_HD uint32_t degree(uint32_t v, const uint32_t* pl_start, const uint32_t* pl_end, const uint64_t* conn_off, const uint32_t* conn_pl) {
  uint32_t d = 0;
  for (uint64_t e = conn_off[v]; e < conn_off[v + 1]; e++) d += pl_start[conn_pl[e]] != pl_end[conn_pl[e]] ? 1u : 0u;
  return d;
}

// The half-edge that follows h (a half-edge of a non-loop polyline) through its far node, kNone at a terminal. deg_far: the
// degree of that node.
EG3D_HD uint32_t successor(uint32_t h, uint32_t deg_far, const uint32_t* pl_start, const uint32_t* pl_end, const uint64_t* conn_off,
                           const uint32_t* conn_pl) {
  if (deg_far != 2) return kNone;
  const uint32_t v = he_far(h, pl_start, pl_end), p = h >> 1;
  for (uint64_t e = conn_off[v]; e < conn_off[v + 1]; e++) {
    const uint32_t q = conn_pl[e];
    if (q == p || pl_start[q] == pl_end[q]) continue;
    return 2u * q + (pl_start[q] == v ? 0u : 1u);
  }
  return kNone;  // (not reached on a checked graph)
}

// Of the two directed lists of a chain, the one the chain is: h is the first half-edge of its list, `last` the last.
EG3D_HD bool head_is_chosen(uint32_t h, uint32_t last) {
  const uint32_t a = h >> 1, b = last >> 1;
  return a < b || (a == b && (h & 1u) == 0u);
}

// ---- the graph's checks, one node's row: returns false when the row is refused. seen[2 p + s] is set for every (polyline,
// end) the row names; `claim` sets a flag and returns its earlier value (atomic on the device).
template <class Claim>
EG3D_HD bool check_row(uint32_t v, uint64_t n_polylines, const uint32_t* pl_start, const uint32_t* pl_end, const uint64_t* conn_off,
                       const uint32_t* conn_pl, Claim& claim, uint32_t* deg_out) {
  uint32_t d = 0;
  bool ok = true;
  for (uint64_t e = conn_off[v]; e < conn_off[v + 1]; e++) {
    const uint32_t p = conn_pl[e];
    if (p >= n_polylines) {
      ok = false;
      continue;
    }
    const uint32_t s = pl_start[p], t = pl_end[p];
    if (s != v && t != v) {
      ok = false;
      continue;
    }
    if (claim(2ull * p + (s != v ? 1u : 0u))) ok = false;  // twice in the row (or in two rows of one node id: impossible)
    d += s != t ? 1u : 0u;
  }
  *deg_out = d;
  return ok;
}

// ---- simplify ------------------------------------------------------------------------------------------------------------
EG3D_HD float distance_point_line_sq(float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = bx - ax, dy = by - ay, dz = bz - az;  // vec6::direction
  const float vx = ax - px, vy = ay - py, vz = az - pz;  // line.start() - p3d
  const float cx = dy * vz - vy * dz;                    // glm::cross(d, v)
  const float cy = dz * vx - vz * dx;
  const float cz = dx * vy - vx * dy;
  return ((cx * cx + cy * cy) + cz * cz) / ((dx * dx + dy * dy) + dz * dz);
}

// linearizable_polyline for one interior point i of (start, end): true when the point REFUSES the line
template <class Pts>
EG3D_HD bool point_off_line(const Pts& P, uint32_t start, uint32_t end, uint32_t i, float maxsq) {
  float a[3], b[3], p[3];
  P.get(start, a);
  P.get(end, b);
  P.get(i, p);
  return distance_point_line_sq(p[0], p[1], p[2], a[0], a[1], a[2], b[0], b[1], b[2]) > maxsq;
}

template <class Lin>
EG3D_HD uint32_t find_max_se(Lin& lin, uint32_t start, uint32_t max_se) {
  if (max_se <= start) return start;
  for (uint32_t cur_se = max_se; cur_se > start + 1; cur_se--)
    if (lin(start, cur_se)) return cur_se;
  return start + 1;
}
template <class Lin>
EG3D_HD uint32_t find_min_eb(Lin& lin, uint32_t end, uint32_t min_eb) {
  if (min_eb >= end) return end;
  for (uint32_t cur_eb = min_eb; cur_eb < end - 1; cur_eb++)
    if (lin(cur_eb, end)) return cur_eb;
  return end - 1;
}
template <class Lin>
EG3D_HD void find_compatible_se_eb(Lin& lin, uint32_t start, uint32_t end, uint32_t* se_out, uint32_t* eb_out) {
  uint32_t se = start, eb = start;
  if (start < end) {
    uint32_t max_se = end, min_eb = start;
    do {
      se = find_max_se(lin, start, max_se);
      if (se == end) {
        eb = 0;
        break;
      }
      eb = find_min_eb(lin, end, min_eb);
      max_se--;
      min_eb++;
    } while (eb < se);
  }
  *se_out = se;
  *eb_out = eb;
}

// simplify_polyline on n >= 2 vertices. lin(start, end): linearizable_polyline. out.front(k, i) / out.back(k, i): vertex i is
// the k-th of the front / of the end list. Returns the two counts.
template <class Lin, class Out>
EG3D_HD void simplify_indices(Lin& lin, uint32_t n, Out& out, uint32_t* nf_out, uint32_t* nb_out) {
  uint32_t start = 0, end = n - 1, nf = 0, nb = 0;
  out.front(nf++, start);
  out.back(nb++, end);
  for (uint32_t round = 0; round < n && end > start + 1; round++) {
    uint32_t se, eb;
    find_compatible_se_eb(lin, start, end, &se, &eb);
    if (se == end) break;  // the whole interval is linearizable
    out.front(nf++, se);
    if (se != eb) out.back(nb++, eb);
    start = se;
    end = eb;
  }
  *nf_out = nf;
  *nb_out = nb;
}

// the vertices of a chain that the simplification sees: all of them, or all but the last of a closed chain (E1)
EG3D_HD uint32_t simplified_span(uint32_t n, uint32_t first_node, uint32_t last_node) { return (n >= 3 && first_node == last_node) ? n - 1 : n; }

// ---- length --------------------------------------------------------------------------------------------------------------
EG3D_HD float distance_3d(const float* a, const float* b) {
  const double dx = (double)(a[0] - b[0]), dy = (double)(a[1] - b[1]), dz = (double)(a[2] - b[2]);
  const float sq = (float)((dx * dx + dy * dy) + dz * dz);
  return EG3D_SQRTF(sq);
}
// the length of the polyline through node_X[node[0 .. n)]
EG3D_HD float polyline_length(const float* node_X, const uint32_t* node, uint64_t n) {
  float length = 0.0f;
  for (uint64_t i = 1; i < n; i++) length += distance_3d(node_X + 3 * (uint64_t)node[i], node_X + 3 * (uint64_t)node[i - 1]);
  return length;
}

}  // namespace edges
}  // namespace eg3d
