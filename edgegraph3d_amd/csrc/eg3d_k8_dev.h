// eg3d_k8_dev.h — the device-side rules of the PLGMatchesManager replay that K8 (eg3d_k8_replay.hip: one cloud) and K8a
// (eg3d_k8a_accumulate.hip: the clouds of a run, one after the other) share: what a chain pair is, when two points are one
// node, and which interval a pair leaves on a view. One copy, so that the two cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_k8_replay.h"

namespace eg3d {

// (i - 1, i) is a chain pair
__device__ __forceinline__ bool k8_is_pair(const CloudView& in, uint64_t i) {
  if (i == 0 || i >= in.n_points) return false;
  const uint32_t* k0 = in.key + 4 * (i - 1);
  const uint32_t* k1 = in.key + 4 * i;
  return k0[0] == k1[0] && k0[1] == k1[1] && k0[2] == k1[2] && k1[3] == k0[3] + 1u;
}
__device__ __forceinline__ bool k8_in_pair(const CloudView& in, uint64_t i) { return k8_is_pair(in, i) || k8_is_pair(in, i + 1); }

// ---- nodes ----
__device__ __forceinline__ uint32_t k8_canon(float f) {
  const uint32_t u = __float_as_uint(f);
  return u == 0x80000000u ? 0u : u;  // -0 == +0
}
struct K8Key {
  uint32_t x, y, z;
};
__device__ __forceinline__ K8Key k8_key(const float* X, uint64_t p) {
  return K8Key{k8_canon(X[3 * p]), k8_canon(X[3 * p + 1]), k8_canon(X[3 * p + 2])};
}
__device__ __forceinline__ uint64_t k8_hash(const K8Key& k) {  // NodeTable::hash of host/replay.cpp
  uint64_t h = 0x9E3779B97F4A7C15ull;
  const uint32_t c[3] = {k.x, k.y, k.z};
#pragma unroll
  for (int q = 0; q < 3; q++) {
    h ^= c[q];
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
  }
  return h;
}
__device__ __forceinline__ bool k8_same(const K8Key& a, const K8Key& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// ---- matched 2-D intervals ----
struct K8Plp {
  uint32_t seg;
  float x, y;
};
// is_ordered_2dlinepoints (geometric_utilities.cpp:1375-1377), as `ordered` of host/replay.cpp
__device__ __forceinline__ bool k8_ordered(float ax, float ay, float bx, float by, float cx, float cy) {
  return (bx - ax) * (cx - bx) > 0 || (by - ay) * (cy - by) > 0 || ((ax == bx && ay == by) || (bx == cx && by == cy));
}
// add_matched_2dsegment: orders (a, b) on polyline gpl into (start, end)
__device__ __forceinline__ void k8_orient(const DevScene& s, uint32_t gpl, K8Plp* a, K8Plp* b) {
  bool swap = a->seg > b->seg;
  if (a->seg == b->seg) {
    const f2 v = s.vtx[(uint64_t)s.pl_vtx_off[gpl] + a->seg];
    swap = !k8_ordered(v.x, v.y, a->x, a->y, b->x, b->y);
  }
  if (swap) {
    const K8Plp t = *a;
    *a = *b;
    *b = t;
  }
}
// The interval of view v between observations o1 (first point) and o2 (second point) of a pair, by
// add_matched_3dsegment (plg_matches_manager.cpp:118-173; host/replay.cpp:229-264). false: none.
__device__ __forceinline__ bool k8_interval(const CloudView& in, const DevScene& s, int32_t v, uint64_t o1, uint64_t o2,
                                            uint32_t* gpl, K8Plp* a, K8Plp* b) {
  *a = K8Plp{in.obs_seg[o1], in.obs_xy[2 * o1], in.obs_xy[2 * o1 + 1]};
  *b = K8Plp{in.obs_seg[o2], in.obs_xy[2 * o2], in.obs_xy[2 * o2 + 1]};
  const uint32_t pl1 = in.obs_pl[o1], pl2 = in.obs_pl[o2];
  const uint32_t g1 = s.view_pl_off[v] + pl1, g2 = s.view_pl_off[v] + pl2;
  if (pl1 != pl2) {
    // different polylines: only if the first point sits on an extreme of its polyline that the second polyline shares
    const uint32_t n1 = s.pl_vtx_off[g1 + 1] - s.pl_vtx_off[g1], n2 = s.pl_vtx_off[g2 + 1] - s.pl_vtx_off[g2];
    const f2* v1 = s.vtx + s.pl_vtx_off[g1];
    const f2* v2 = s.vtx + s.pl_vtx_off[g2];
    uint32_t node_id = 0;
    bool extreme = false;
    if (a->seg == 0 && a->x == v1[0].x && a->y == v1[0].y) {  // is_start
      node_id = s.pl_start[g1];
      extreme = true;
    }
    if (!extreme && a->seg == n1 - 2 && a->x == v1[n1 - 1].x && a->y == v1[n1 - 1].y) {  // is_end
      node_id = s.pl_end[g1];
      extreme = true;
    }
    if (!extreme) return false;
    if (node_id == s.pl_start[g2])
      *a = K8Plp{0u, v2[0].x, v2[0].y};
    else if (node_id == s.pl_end[g2])
      *a = K8Plp{n2 - 2, v2[n2 - 1].x, v2[n2 - 1].y};
    else
      return false;
  }
  *gpl = g2;
  k8_orient(s, g2, a, b);
  return true;
}

}  // namespace eg3d
