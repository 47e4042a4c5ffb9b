// Host replay of the PLGMatchesManager side effects of the path.
//
// The reference records every emitted chain while it runs: plgmm.add_matched_3dpolyline(chain)
// (src/edgegraph3d/matching/plg_matching/plg_matching_from_refpoints.cpp:74-77) turns each
// consecutive pair of chain points into a direct connection of the 3-D polyline graph
// (plg_matches_manager.cpp:110-116, polyline_graph_3d_hmap_impl.cpp:47-68,121-141) and marks the 2-D
// interval between their observations as matched on every view both points see
// (plg_matches_manager.cpp:99-108,118-173). On this path the manager is write-only, so the GPU
// never needs it; this file rebuilds it afterwards from the ordered edge-point cloud (the chain
// boundaries are in `key`), in one pass, with flat arrays instead of the reference's hash map of
// glm::vec3 / vector-of-vectors / std::set per polyline:
//   * node lookup: open-addressing table over the canonical bit pattern of (x,y,z) — the
//     reference's key equality is float ==, so -0 and +0 are one key and a NaN never matches;
//   * connections of a node: singly linked lists in two flat arrays (insertion order kept);
//   * matched intervals: the reference's std::set orders intervals by start.segment_index ONLY, so a
//     second interval starting on the same segment of the same polyline is silently dropped — kept
//     here as "first insertion wins" through a hash set of (polyline, start segment).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <unordered_set>
#include <vector>

#include "../../include/eg3d_host.h"
#include "../../include/eg3d_host_accumulate.h"
#include "../../include/eg3d_host_replay_merge.h"

namespace {

const float kInvalid = -1.0f;  // INVALID_POINT_COORDS (polyline_graph_3d.hpp:57)

struct NodeTable {
  std::vector<uint32_t> slot;  // node id + 1, 0 = empty
  std::vector<float> key;      // [slots][3] the coordinates the slot was inserted with
  uint64_t mask = 0;
  uint64_t used = 0;  // occupied slots
  // Room for `more` further insertions with at least half the slots free: the table of one cloud of n points (two
  // insertions per point at the most: a NaN point makes a node per lookup) is what it was when a replay took one cloud;
  // a state that accumulates grows it by rehashing the stored keys (a NaN key parks at a free slot again).
  void reserve(uint64_t more) {
    uint64_t cap = slot.empty() ? 64 : slot.size();
    while (cap < (used + more) * 2 + 16) cap <<= 1;
    if (cap == slot.size()) return;
    std::vector<uint32_t> old_slot(cap, 0);
    std::vector<float> old_key(cap * 3, 0.f);
    old_slot.swap(slot);
    old_key.swap(key);
    mask = cap - 1;
    for (size_t i = 0; i < old_slot.size(); i++) {
      if (!old_slot[i]) continue;
      bool found;
      const uint64_t j = find(&old_key[i * 3], found);
      slot[j] = old_slot[i];
      memcpy(&key[j * 3], &old_key[i * 3], 3 * sizeof(float));
    }
  }
  static uint32_t canon(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u == 0x80000000u ? 0u : u;  // -0 == +0
  }
  static uint64_t hash(const float* X) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < 3; k++) {
      h ^= canon(X[k]);
      h *= 0xBF58476D1CE4E5B9ull;
      h ^= h >> 29;
    }
    return h;
  }
  // slot index holding X, or the empty slot where it would go (found = false)
  uint64_t find(const float* X, bool& found) const {
    found = false;
    if (X[0] != X[0] || X[1] != X[1] || X[2] != X[2]) {  // NaN: equal to nothing; park at any empty slot
      uint64_t i = hash(X) & mask;
      while (slot[i]) i = (i + 1) & mask;
      return i;
    }
    uint64_t i = hash(X) & mask;
    while (slot[i]) {
      const float* k = &key[i * 3];
      if (k[0] == X[0] && k[1] == X[1] && k[2] == X[2]) {
        found = true;
        return i;
      }
      i = (i + 1) & mask;
    }
    return i;
  }
};

struct Plp {
  uint32_t seg;
  float x, y;
};

// is_ordered_2dlinepoints (geometric_utilities.cpp:1375-1377)
bool ordered(float ax, float ay, float bx, float by, float cx, float cy) {
  return (bx - ax) * (cx - bx) > 0 || (by - ay) * (cy - by) > 0 || ((ax == bx && ay == by) || (bx == cx && by == cy));
}

}  // namespace

// The manager itself: everything the replay of one cloud used to keep on its stack lives here, so that the clouds of a
// run can be added one after the other (include/eg3d_host_accumulate.h). Points are numbered through the run (n_points
// added so far + the index within the cloud): node_point holds those numbers, and every first-claim rule below sees the
// earlier clouds' claims standing. eg3d_host_replay_matches is one state that takes one cloud.
struct eg3d_replay_state {
  const eg3d_scene* sc = nullptr;
  NodeTable table;
  std::vector<float> node_X;
  std::vector<uint64_t> node_point;
  std::vector<uint32_t> head, tail, cnt;      // per node: connection list
  std::vector<uint32_t> link_pl, link_next;   // list cells
  std::vector<uint32_t> pl_s, pl_e;
  uint64_t real_nodes = 0;
  struct Iv {
    uint32_t gpl, s_seg, e_seg;
    float sx, sy, ex, ey;
  };
  std::vector<Iv> ivs;
  std::unordered_set<uint64_t> iv_keys;
  uint64_t n_points = 0;     // points of the clouds added so far
  uint32_t last_key[4] = {0, 0, 0, 0};  // key of the last point added (a cloud that would continue its chain is refused)
  bool have_last = false;
  int add(const eg3d_edgepoints* pts);
  int merge(const eg3d_graph3d* later, uint64_t later_points);
  int graph(eg3d_graph3d* out);
};

int eg3d_replay_state::add(const eg3d_edgepoints* pts) {
  if (!pts) return -1;
  const int V = sc->n_views;
  const uint64_t N = pts->n_points;
  const uint64_t base = n_points;
  if (N >= 0xfffffff0ull || base + N >= 0xfffffff0ull) return -3;  // node / polyline ids are 32-bit here (documented narrowing)
  // the cloud normally comes from eg3d_match_*; one built by the caller is checked before its ids index the scene
  if (N && (!pts->X || !pts->obs_off || !pts->key)) return -1;
  for (uint64_t p = 0; p < N; p++)
    if (pts->obs_off[p + 1] < pts->obs_off[p] || pts->obs_off[p + 1] > pts->n_obs) return -1;
  if (N && pts->obs_off[N] && (!pts->obs_view || !pts->obs_pl || !pts->obs_seg || !pts->obs_xy)) return -1;
  for (uint64_t o = 0, no = N ? pts->obs_off[N] : 0; o < no; o++) {
    const int32_t v = pts->obs_view[o];
    if (v < 0 || v >= V) return -1;
    const uint32_t npl = sc->view_pl_off[v + 1] - sc->view_pl_off[v];
    if (pts->obs_pl[o] >= npl) return -1;
    const uint32_t g = sc->view_pl_off[v] + pts->obs_pl[o];
    const uint32_t nv = sc->pl_vtx_off[g + 1] - sc->pl_vtx_off[g];
    if (nv < 2 || pts->obs_seg[o] >= nv - 1) return -1;  // a segment index of a polyline that has segments
  }
  // a cloud is made of whole chains: one whose first point continues the chain the last cloud ended on is refused
  if (N && have_last && pts->key[0] == last_key[0] && pts->key[1] == last_key[1] && pts->key[2] == last_key[2] &&
      pts->key[3] == last_key[3] + 1)
    return -1;
  // ---- nothing was changed up to here; from here on nothing fails
  if (!N) return 0;
  table.reserve(N);
  n_points = base + N;
  memcpy(last_key, pts->key + 4 * (N - 1), sizeof(last_key));
  have_last = true;

  auto node_valid = [&](uint32_t id) { return node_X[3 * (size_t)id] != kInvalid && node_X[3 * (size_t)id + 1] != kInvalid; };
  auto new_node = [&](const float* X) {
    const uint32_t id = (uint32_t)node_point.size();
    node_X.insert(node_X.end(), X, X + 3);
    node_point.push_back(~0ull);
    head.push_back(~0u);
    tail.push_back(~0u);
    cnt.push_back(0);
    real_nodes++;
    return id;
  };
  // get_node_id (polyline_graph_3d_hmap_impl.cpp:47-68)
  auto node_of = [&](const float* X) {
    bool found;
    const uint64_t i = table.find(X, found);
    if (found) {
      const uint32_t id = table.slot[i] - 1;
      if (node_valid(id)) return id;
      // a node whose x or y equals INVALID_POINT_COORDS is "invalid": wiped, and a fresh node takes the key
      node_X[3 * (size_t)id] = node_X[3 * (size_t)id + 1] = node_X[3 * (size_t)id + 2] = kInvalid;
      head[id] = tail[id] = ~0u;
      cnt[id] = 0;
      const uint32_t nid = new_node(X);
      table.slot[i] = nid + 1;
      return nid;
    }
    const uint32_t id = new_node(X);
    table.used++;
    table.slot[i] = id + 1;
    table.key[i * 3] = X[0];
    table.key[i * 3 + 1] = X[1];
    table.key[i * 3 + 2] = X[2];
    return id;
  };
  auto connect = [&](uint32_t node, uint32_t pl) {
    const uint32_t cell = (uint32_t)link_pl.size();
    link_pl.push_back(pl);
    link_next.push_back(~0u);
    if (tail[node] == ~0u)
      head[node] = cell;
    else
      link_next[tail[node]] = cell;
    tail[node] = cell;
    cnt[node]++;
  };
  // add_direct_connection(start, end) -> internal_add_polyline unless is_duplicate (:99-127)
  auto add_connection = [&](uint32_t a, uint32_t b) {
    const uint32_t scan = cnt[a] < cnt[b] ? a : b;  // "smallest_connections": s unless e is strictly smaller
    const uint32_t from = cnt[a] < cnt[b] ? a : b;
    (void)from;
    for (uint32_t c = head[scan]; c != ~0u; c = link_next[c]) {
      const uint32_t p = link_pl[c];
      // polyline equality: same extremes (either orientation) and the same two coordinates — which
      // are the extremes' node coordinates, compared with float == (a NaN coordinate never matches)
      const bool same = (pl_s[p] == a && pl_e[p] == b) || (pl_s[p] == b && pl_e[p] == a);
      if (!same) continue;
      const float* xa = &node_X[3 * (size_t)a];
      const float* xb = &node_X[3 * (size_t)b];
      if (xa[0] == xa[0] && xa[1] == xa[1] && xa[2] == xa[2] && xb[0] == xb[0] && xb[1] == xb[1] && xb[2] == xb[2]) return;
    }
    const uint32_t id = (uint32_t)pl_s.size();
    pl_s.push_back(a);
    pl_e.push_back(b);
    connect(a, id);
    if (a != b) connect(b, id);
  };

  // matched 2-D intervals
  auto insert_iv = [&](uint32_t gpl, const Plp& a, const Plp& b) {
    if (!iv_keys.insert(((uint64_t)gpl << 32) | a.seg).second) return;  // std::set keyed on start.segment_index
    ivs.push_back({gpl, a.seg, b.seg, a.x, a.y, b.x, b.y});
  };
  // add_matched_2dsegment (plg_matches_manager.cpp:99-108)
  auto add_2dsegment = [&](int view, uint32_t pl, const Plp& a, const Plp& b) {
    const uint32_t gpl = sc->view_pl_off[view] + pl;
    if (a.seg < b.seg)
      insert_iv(gpl, a, b);
    else if (a.seg > b.seg)
      insert_iv(gpl, b, a);
    else {
      const float* v = sc->vtx_xy + 2 * ((size_t)sc->pl_vtx_off[gpl] + a.seg);
      if (ordered(v[0], v[1], a.x, a.y, b.x, b.y))
        insert_iv(gpl, a, b);
      else
        insert_iv(gpl, b, a);
    }
  };

  std::vector<int64_t> slot1((size_t)V), slot2((size_t)V);  // observation index of each view in p1 / p2, -1 = unseen
  for (uint64_t i = 1; i < N; i++) {
    const uint32_t* k0 = pts->key + 4 * (i - 1);
    const uint32_t* k1 = pts->key + 4 * i;
    if (k0[0] != k1[0] || k0[1] != k1[1] || k0[2] != k1[2] || k1[3] != k0[3] + 1) continue;  // first point of a chain
    // ---- add_matched_3dsegment(p[i-1], p[i]) (plg_matches_manager.cpp:110-173)
    const uint32_t na = node_of(pts->X + 3 * (i - 1));
    const uint32_t nb = node_of(pts->X + 3 * i);
    add_connection(na, nb);
    node_point[na] = base + i - 1;  // set_observations: last writer wins (first, then second)
    node_point[nb] = base + i;
    std::fill(slot1.begin(), slot1.end(), -1);
    std::fill(slot2.begin(), slot2.end(), -1);
    for (uint64_t o = pts->obs_off[i - 1]; o < pts->obs_off[i]; o++) slot1[pts->obs_view[o]] = (int64_t)o;
    for (uint64_t o = pts->obs_off[i]; o < pts->obs_off[i + 1]; o++) slot2[pts->obs_view[o]] = (int64_t)o;
    for (int v = 0; v < V; v++) {
      if (slot1[v] < 0 || slot2[v] < 0) continue;
      const uint64_t o1 = (uint64_t)slot1[v], o2 = (uint64_t)slot2[v];
      const Plp a = {pts->obs_seg[o1], pts->obs_xy[2 * o1], pts->obs_xy[2 * o1 + 1]};
      const Plp b = {pts->obs_seg[o2], pts->obs_xy[2 * o2], pts->obs_xy[2 * o2 + 1]};
      const uint32_t pl1 = pts->obs_pl[o1], pl2 = pts->obs_pl[o2];
      if (pl1 == pl2) {
        add_2dsegment(v, pl1, a, b);
        continue;
      }
      // different polylines: only if the first point sits on an extreme of its polyline that the
      // second polyline shares (:132-164)
      const uint32_t g1 = sc->view_pl_off[v] + pl1, g2 = sc->view_pl_off[v] + pl2;
      const uint32_t n1 = sc->pl_vtx_off[g1 + 1] - sc->pl_vtx_off[g1];
      const float* v1 = sc->vtx_xy + 2 * (size_t)sc->pl_vtx_off[g1];
      if (n1 < 2) continue;
      uint32_t node_id = 0;
      bool extreme = false;
      if (a.seg == 0 && a.x == v1[0] && a.y == v1[1]) {  // is_start(plp)
        node_id = sc->pl_start[g1];
        extreme = true;
      }
      if (!extreme && a.seg == n1 - 2 && a.x == v1[2 * (n1 - 1)] && a.y == v1[2 * (n1 - 1) + 1]) {  // is_end(plp)
        node_id = sc->pl_end[g1];
        extreme = true;
      }
      if (!extreme) continue;
      const uint32_t n2 = sc->pl_vtx_off[g2 + 1] - sc->pl_vtx_off[g2];
      const float* v2 = sc->vtx_xy + 2 * (size_t)sc->pl_vtx_off[g2];
      if (n2 < 2) continue;
      Plp ext;
      if (node_id == sc->pl_start[g2])  // get_extreme_plp(node_id, valid) (polyline_graph_2d.cpp:151-160)
        ext = {0u, v2[0], v2[1]};
      else if (node_id == sc->pl_end[g2])
        ext = {n2 - 2, v2[2 * (n2 - 1)], v2[2 * (n2 - 1) + 1]};
      else
        continue;
      add_2dsegment(v, pl2, ext, b);
    }
  }
  return 0;
}

// ---- the graph of the run that follows directly, in place of its cloud (include/eg3d_host_replay_merge.h states the rule)
int eg3d_replay_state::merge(const eg3d_graph3d* B, uint64_t nB) {
  if (!B) return -1;
  const uint64_t nA = n_points;
  if (nB >= 0xfffffff0ull || nA + nB >= 0xfffffff0ull) return -3;
  const uint32_t NP = sc->view_pl_off[sc->n_views];
  const uint64_t NN = B->n_nodes, NL = B->n_polylines;
  if (B->n_scene_polylines != NP || !B->iv_off) return -1;
  if (NN > nB || NL > nB) return -1;  // every node has a point of its own, every polyline a pair of its own
  if ((NN && (!B->node_X || !B->node_point)) || (NL && (!B->pl_start || !B->pl_end))) return -1;
  auto segments = [&](uint32_t g) {
    const uint32_t nv = sc->pl_vtx_off[g + 1] - sc->pl_vtx_off[g];
    return nv < 2 ? 0u : nv - 1;
  };
  // ---- the checks: nothing of B is used as an index before it is known to be one, and nothing of the state changes
  for (uint64_t n = 0; n < NN; n++)
    if (B->node_point[n] >= nB) return -1;
  for (uint64_t j = 0; j < NL; j++)
    if (B->pl_start[j] >= NN || B->pl_end[j] >= NN) return -1;
  if (B->iv_off[0] != 0) return -1;
  for (uint32_t g = 0; g < NP; g++)
    if (B->iv_off[g] > B->iv_off[g + 1] || B->iv_off[g + 1] - B->iv_off[g] > segments(g)) return -1;
  const uint64_t NI = B->iv_off[NP];
  if (NI && (!B->iv_start_seg || !B->iv_end_seg || !B->iv_start_xy || !B->iv_end_xy)) return -1;
  for (uint32_t g = 0; g < NP; g++)
    for (uint64_t k = B->iv_off[g]; k < B->iv_off[g + 1]; k++) {
      if (B->iv_start_seg[k] >= segments(g) || B->iv_end_seg[k] >= segments(g)) return -1;
      if (k > B->iv_off[g] && B->iv_start_seg[k - 1] >= B->iv_start_seg[k]) return -1;
    }
  {
    std::unordered_set<uint64_t> pairs;
    for (uint64_t j = 0; j < NL; j++) {
      const uint32_t a = B->pl_start[j], b = B->pl_end[j];
      if (!pairs.insert(((uint64_t)(a < b ? a : b) << 32) | (a < b ? b : a)).second) return -1;
    }
    NodeTable own;  // B's nodes among themselves, by the bit patterns (a NaN is refused below, after every -1)
    own.reserve(NN);
    for (uint64_t n = 0; n < NN; n++) {
      uint64_t i = NodeTable::hash(B->node_X + 3 * n) & own.mask;
      for (; own.slot[i]; i = (i + 1) & own.mask) {
        const float* k = B->node_X + 3 * (size_t)(own.slot[i] - 1);
        if (NodeTable::canon(k[0]) == NodeTable::canon(B->node_X[3 * n]) && NodeTable::canon(k[1]) == NodeTable::canon(B->node_X[3 * n + 1]) &&
            NodeTable::canon(k[2]) == NodeTable::canon(B->node_X[3 * n + 2]))
          return -1;
      }
      own.slot[i] = (uint32_t)n + 1;
    }
  }
  auto plain = [](const float* X) { return X[0] == X[0] && X[1] == X[1] && X[2] == X[2] && X[0] != kInvalid && X[1] != kInvalid; };
  if (B->n_real_nodes != NN || real_nodes != node_point.size()) return -5;
  for (uint64_t n = 0; n < NN; n++)
    if (!plain(B->node_X + 3 * n)) return -5;
  for (size_t n = 0; n < node_point.size(); n++)
    if (!plain(&node_X[3 * n])) return -5;
  // ---- nothing was changed up to here; from here on nothing fails
  n_points = nA + nB;
  if (nB) have_last = false;  // a graph does not carry the key its cloud ended on: the next cloud is not checked against it
  table.reserve(NN);
  std::vector<uint32_t> id_of((size_t)NN);
  for (uint64_t n = 0; n < NN; n++) {
    const float* X = B->node_X + 3 * n;
    bool found;
    const uint64_t i = table.find(X, found);
    if (found)
      id_of[n] = table.slot[i] - 1;  // A's node: its node_X stands
    else {
      id_of[n] = (uint32_t)node_point.size();
      node_X.insert(node_X.end(), X, X + 3);
      node_point.push_back(~0ull);
      head.push_back(~0u);
      tail.push_back(~0u);
      cnt.push_back(0);
      real_nodes++;
      table.used++;
      table.slot[i] = id_of[n] + 1;
      memcpy(&table.key[i * 3], X, 3 * sizeof(float));
    }
    node_point[id_of[n]] = nA + B->node_point[n];  // B's points all come after A's: last writer
  }
  auto connect = [&](uint32_t node, uint32_t pl) {
    const uint32_t cell = (uint32_t)link_pl.size();
    link_pl.push_back(pl);
    link_next.push_back(~0u);
    if (tail[node] == ~0u)
      head[node] = cell;
    else
      link_next[tail[node]] = cell;
    tail[node] = cell;
    cnt[node]++;
  };
  for (uint64_t j = 0; j < NL; j++) {
    const uint32_t a = id_of[B->pl_start[j]], b = id_of[B->pl_end[j]];
    bool held = false;
    for (uint32_t c = head[cnt[a] < cnt[b] ? a : b]; c != ~0u && !held; c = link_next[c]) {
      const uint32_t p = link_pl[c];
      held = (pl_s[p] == a && pl_e[p] == b) || (pl_s[p] == b && pl_e[p] == a);
    }
    if (held) continue;  // A's polyline: id and orientation stand
    const uint32_t id = (uint32_t)pl_s.size();
    pl_s.push_back(a);
    pl_e.push_back(b);
    connect(a, id);
    if (a != b) connect(b, id);
  }
  for (uint32_t g = 0; g < NP; g++)
    for (uint64_t k = B->iv_off[g]; k < B->iv_off[g + 1]; k++) {
      if (!iv_keys.insert(((uint64_t)g << 32) | B->iv_start_seg[k]).second) continue;  // A's record stands
      ivs.push_back({g, B->iv_start_seg[k], B->iv_end_seg[k], B->iv_start_xy[2 * k], B->iv_start_xy[2 * k + 1], B->iv_end_xy[2 * k],
                     B->iv_end_xy[2 * k + 1]});
    }
  return 0;
}

// ---- flatten: a snapshot; the state is as it was (the order of `ivs` carries nothing: iv_keys decides the claims)
int eg3d_replay_state::graph(eg3d_graph3d* out) {
  if (!out) return -1;
  memset(out, 0, sizeof(*out));
  const uint32_t NP = sc->view_pl_off[sc->n_views];
  const uint64_t NN = node_point.size();
  out->n_nodes = NN;
  out->n_real_nodes = real_nodes;
  out->n_polylines = pl_s.size();
  out->n_scene_polylines = NP;
  auto dup = [](const void* src, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (bytes) memcpy(p, src, bytes);
    return p;
  };
  out->node_X = (float*)dup(node_X.data(), sizeof(float) * node_X.size());
  out->node_point = (uint64_t*)dup(node_point.data(), sizeof(uint64_t) * NN);
  out->pl_start = (uint32_t*)dup(pl_s.data(), sizeof(uint32_t) * pl_s.size());
  out->pl_end = (uint32_t*)dup(pl_e.data(), sizeof(uint32_t) * pl_e.size());
  out->conn_off = (uint64_t*)malloc(sizeof(uint64_t) * (NN + 1));
  out->conn_pl = (uint32_t*)malloc(sizeof(uint32_t) * (link_pl.size() + 1));
  uint64_t w = 0;
  for (uint64_t n = 0; n < NN; n++) {
    out->conn_off[n] = w;
    for (uint32_t c = head[n]; c != ~0u; c = link_next[c]) out->conn_pl[w++] = link_pl[c];
  }
  out->conn_off[NN] = w;
  std::sort(ivs.begin(), ivs.end(), [](const Iv& a, const Iv& b) { return a.gpl != b.gpl ? a.gpl < b.gpl : a.s_seg < b.s_seg; });
  const uint64_t NI = ivs.size();
  out->iv_off = (uint64_t*)calloc((size_t)NP + 1, sizeof(uint64_t));
  out->iv_start_seg = (uint32_t*)malloc(sizeof(uint32_t) * (NI + 1));
  out->iv_end_seg = (uint32_t*)malloc(sizeof(uint32_t) * (NI + 1));
  out->iv_start_xy = (float*)malloc(sizeof(float) * 2 * (NI + 1));
  out->iv_end_xy = (float*)malloc(sizeof(float) * 2 * (NI + 1));
  for (uint64_t k = 0; k < NI; k++) {
    out->iv_off[ivs[k].gpl + 1]++;
    out->iv_start_seg[k] = ivs[k].s_seg;
    out->iv_end_seg[k] = ivs[k].e_seg;
    out->iv_start_xy[2 * k] = ivs[k].sx;
    out->iv_start_xy[2 * k + 1] = ivs[k].sy;
    out->iv_end_xy[2 * k] = ivs[k].ex;
    out->iv_end_xy[2 * k + 1] = ivs[k].ey;
  }
  for (uint32_t p = 0; p < NP; p++) out->iv_off[p + 1] += out->iv_off[p];
  return 0;
}

extern "C" eg3d_replay_state* eg3d_host_replay_state_create(const eg3d_scene* sc) {
  if (!sc || sc->n_views < 1 || !sc->view_pl_off || !sc->pl_vtx_off || !sc->vtx_xy) return nullptr;
  eg3d_replay_state* s = new (std::nothrow) eg3d_replay_state;
  if (s) s->sc = sc;
  return s;
}
extern "C" int eg3d_host_replay_state_add(eg3d_replay_state* s, const eg3d_edgepoints* pts) { return s ? s->add(pts) : -1; }
extern "C" int eg3d_host_replay_state_merge_graph(eg3d_replay_state* s, const eg3d_graph3d* later, uint64_t later_points) {
  return s ? s->merge(later, later_points) : -1;
}
extern "C" int eg3d_host_replay_state_graph(eg3d_replay_state* s, eg3d_graph3d* out) { return s ? s->graph(out) : -1; }
extern "C" uint64_t eg3d_host_replay_state_points(const eg3d_replay_state* s) { return s ? s->n_points : 0; }
extern "C" void eg3d_host_replay_state_destroy(eg3d_replay_state* s) { delete s; }

extern "C" int eg3d_host_replay_matches(const eg3d_scene* sc, const eg3d_edgepoints* pts, eg3d_graph3d* out) {
  if (!sc || !pts || !out) return -1;
  memset(out, 0, sizeof(*out));
  eg3d_replay_state* s = eg3d_host_replay_state_create(sc);
  if (!s) return -1;
  int rc = s->add(pts);
  if (rc == 0) rc = s->graph(out);
  delete s;
  return rc;
}

extern "C" void eg3d_host_free_graph3d(eg3d_graph3d* g) {
  if (!g) return;
  free(g->node_X);
  free(g->node_point);
  free(g->pl_start);
  free(g->pl_end);
  free(g->conn_off);
  free(g->conn_pl);
  free(g->iv_off);
  free(g->iv_start_seg);
  free(g->iv_end_seg);
  free(g->iv_start_xy);
  free(g->iv_end_xy);
  memset(g, 0, sizeof(*g));
}
