// eg3d_host_replay_state_merge_graph (include/eg3d_host_replay_merge.h) without a GPU and without Python: a run of 40 small
// clouds is folded three ways — the clouds added to one state, the graphs of the separate replays merged into a second, and
// the graphs of the two halves (each a fold of its own) merged into a third — and all three must hold the same bytes after
// every step, which must be the bytes of eg3d_host_replay_matches on the concatenation. Refused graphs in between must change
// nothing. Stand-alone, so that it can be built with the host sources under -fsanitize=address,undefined and run as it is:
//   g++ -std=c++17 -O1 -g -fopenmp -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include
//       -I edgegraph3d_amd/csrc tests/refapi/replay_merge_check.cpp edgegraph3d_amd/host/*.cpp -lz -o replay_merge_check
// (tests/test_replay_merge.py builds it against libeg3d_host.so, without the sanitizers, and runs it.)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "eg3d_host.h"
#include "eg3d_host_accumulate.h"
#include "eg3d_host_replay_merge.h"

static bool same(const eg3d_graph3d& a, const eg3d_graph3d& b) {
  if (a.n_nodes != b.n_nodes || a.n_real_nodes != b.n_real_nodes || a.n_polylines != b.n_polylines ||
      a.n_scene_polylines != b.n_scene_polylines)
    return false;
  const uint64_t nc = a.conn_off[a.n_nodes], ni = a.iv_off[a.n_scene_polylines];
  if (nc != b.conn_off[b.n_nodes] || ni != b.iv_off[b.n_scene_polylines]) return false;
  return !memcmp(a.node_X, b.node_X, 12 * a.n_nodes) && !memcmp(a.node_point, b.node_point, 8 * a.n_nodes) &&
         !memcmp(a.pl_start, b.pl_start, 4 * a.n_polylines) && !memcmp(a.pl_end, b.pl_end, 4 * a.n_polylines) &&
         !memcmp(a.conn_off, b.conn_off, 8 * (a.n_nodes + 1)) && !memcmp(a.conn_pl, b.conn_pl, 4 * nc) &&
         !memcmp(a.iv_off, b.iv_off, 8 * (a.n_scene_polylines + 1)) && !memcmp(a.iv_start_seg, b.iv_start_seg, 4 * ni) &&
         !memcmp(a.iv_end_seg, b.iv_end_seg, 4 * ni) && !memcmp(a.iv_start_xy, b.iv_start_xy, 8 * ni) &&
         !memcmp(a.iv_end_xy, b.iv_end_xy, 8 * ni);
}

// a cloud that owns its arrays
struct Cloud {
  std::vector<float> X, xy;
  std::vector<uint64_t> off = {0};
  std::vector<int32_t> view;
  std::vector<uint32_t> pl, seg, key;
  void point(const float* x, uint32_t p, uint32_t s, const float* at, uint32_t chain, uint32_t k) {
    X.insert(X.end(), x, x + 3);
    view.push_back(0), pl.push_back(p), seg.push_back(s);
    xy.insert(xy.end(), at, at + 2);
    off.push_back(view.size());
    const uint32_t k4[4] = {chain, 0, 0, k};
    key.insert(key.end(), k4, k4 + 4);
  }
  void append(const Cloud& o) {
    const uint64_t base = view.size();
    X.insert(X.end(), o.X.begin(), o.X.end());
    xy.insert(xy.end(), o.xy.begin(), o.xy.end());
    view.insert(view.end(), o.view.begin(), o.view.end());
    pl.insert(pl.end(), o.pl.begin(), o.pl.end());
    seg.insert(seg.end(), o.seg.begin(), o.seg.end());
    key.insert(key.end(), o.key.begin(), o.key.end());
    for (size_t i = 1; i < o.off.size(); i++) off.push_back(base + o.off[i]);
  }
  eg3d_edgepoints c() {
    eg3d_edgepoints e;
    memset(&e, 0, sizeof(e));
    e.n_points = off.size() - 1, e.n_obs = view.size();
    e.X = X.data(), e.obs_off = off.data(), e.obs_view = view.data(), e.obs_pl = pl.data(), e.obs_seg = seg.data();
    e.obs_xy = xy.data(), e.key = key.data();
    return e;
  }
};

int main() {
  eg3d_synth_config cfg;
  eg3d_synth_default_config(&cfg, 0);
  eg3d_synth* syn = eg3d_synth_create(&cfg);
  const eg3d_scene& sc = *eg3d_synth_scene(syn);
  uint32_t pl = 0;  // view 0's first polyline with three segments
  while (sc.pl_vtx_off[pl + 1] - sc.pl_vtx_off[pl] < 4) pl++;
  const float* v0 = sc.vtx_xy + 2 * sc.pl_vtx_off[pl];
  int bad = 0;
  const int ROUNDS = 40;  // (enough nodes for the table to grow several times)
  // round r: two chains. Every second round repeats the nodes of the one before, a connection in the other orientation and
  // the start segments of its intervals; one node is shared by all rounds, as -0.0 and as +0.0 in turn
  std::vector<Cloud> parts(ROUNDS);
  for (int r = 0; r < ROUNDS; r++) {
    const float s = 16.f * (float)(r / 2), z = (r & 1) ? -0.0f : 0.0f;
    const float A[3] = {1 + s, 2, 3}, B[3] = {4 + s, 5, 6}, Cc[3] = {7 + s, 8, 9}, Z[3] = {z, 0, 1};
    if (r & 1) {
      parts[r].point(B, pl, 0, v0, 2 * r, 0), parts[r].point(A, pl, 2, v0 + 4, 2 * r, 1), parts[r].point(Z, pl, 1, v0 + 2, 2 * r, 2);
      parts[r].point(Cc, pl, 1, v0 + 2, 2 * r + 1, 0);
    } else {
      parts[r].point(A, pl, 0, v0, 2 * r, 0), parts[r].point(B, pl, 1, v0 + 2, 2 * r, 1);
      parts[r].point(Cc, pl, 2, v0 + 4, 2 * r + 1, 0), parts[r].point(A, pl, 1, v0 + 2, 2 * r + 1, 1), parts[r].point(Z, pl, 1, v0 + 2, 2 * r + 1, 2);
    }
  }
  eg3d_replay_state* by_cloud = eg3d_host_replay_state_create(&sc);
  eg3d_replay_state* by_graph = eg3d_host_replay_state_create(&sc);
  eg3d_replay_state* halves[2] = {eg3d_host_replay_state_create(&sc), eg3d_host_replay_state_create(&sc)};
  if (!by_cloud || !by_graph || !halves[0] || !halves[1]) bad |= 1;
  Cloud all;
  uint64_t half_points[2] = {0, 0};
  for (int r = 0; r < ROUNDS && !bad; r++) {
    eg3d_edgepoints e = parts[r].c();
    eg3d_graph3d g, want, ga, gb;
    if (eg3d_host_replay_matches(&sc, &e, &g) != 0) bad |= 2;
    if (eg3d_host_replay_state_add(by_cloud, &e) != 0) bad |= 4;
    // refused in between: an endpoint that is no node (-1), a NaN coordinate (-5), the two together (-1), too few points (-1)
    if (g.n_polylines && g.n_nodes) {
      const uint32_t keep_end = g.pl_end[0];
      const float keep_x = g.node_X[2];
      g.pl_end[0] = (uint32_t)g.n_nodes;
      if (eg3d_host_replay_state_merge_graph(by_graph, &g, e.n_points) != -1) bad |= 8;
      g.node_X[2] = NAN;
      if (eg3d_host_replay_state_merge_graph(by_graph, &g, e.n_points) != -1) bad |= 8;
      g.pl_end[0] = keep_end;
      if (eg3d_host_replay_state_merge_graph(by_graph, &g, e.n_points) != -5) bad |= 16;
      g.node_X[2] = keep_x;
      if (eg3d_host_replay_state_merge_graph(by_graph, &g, 1) != -1) bad |= 32;
      if (eg3d_host_replay_state_merge_graph(by_graph, &g, 0xfffffff0ull) != -3) bad |= 32;
    }
    if (eg3d_host_replay_state_merge_graph(by_graph, &g, e.n_points) != 0) bad |= 64;
    const int h = r < ROUNDS / 2 ? 0 : 1;
    if (eg3d_host_replay_state_merge_graph(halves[h], &g, e.n_points) != 0) bad |= 64;
    half_points[h] += e.n_points;
    all.append(parts[r]);
    eg3d_edgepoints ea = all.c();
    if (eg3d_host_replay_matches(&sc, &ea, &want) != 0) bad |= 128;
    if (eg3d_host_replay_state_graph(by_cloud, &ga) != 0 || eg3d_host_replay_state_graph(by_graph, &gb) != 0) bad |= 256;
    if (!bad && (!same(ga, want) || !same(gb, want))) bad |= 512;
    if (eg3d_host_replay_state_points(by_graph) != ea.n_points) bad |= 1024;
    eg3d_host_free_graph3d(&g), eg3d_host_free_graph3d(&want), eg3d_host_free_graph3d(&ga), eg3d_host_free_graph3d(&gb);
  }
  // the pairwise step: the graphs of the two halves, each a fold of its own, into an empty state
  if (!bad) {
    eg3d_replay_state* top = eg3d_host_replay_state_create(&sc);
    eg3d_graph3d g0, g1, gt, want;
    eg3d_edgepoints ea = all.c();
    if (eg3d_host_replay_state_graph(halves[0], &g0) != 0 || eg3d_host_replay_state_graph(halves[1], &g1) != 0) bad |= 2048;
    if (eg3d_host_replay_state_merge_graph(top, &g0, half_points[0]) != 0) bad |= 4096;
    if (eg3d_host_replay_state_graph(top, &gt) != 0 || !same(gt, g0)) bad |= 8192;  // into an empty state: the graph itself
    eg3d_host_free_graph3d(&gt);
    if (eg3d_host_replay_state_merge_graph(top, &g1, half_points[1]) != 0) bad |= 4096;
    if (eg3d_host_replay_matches(&sc, &ea, &want) != 0 || eg3d_host_replay_state_graph(top, &gt) != 0 || !same(gt, want)) bad |= 16384;
    if (g0.n_nodes + g1.n_nodes <= want.n_nodes) bad |= 32768;  // (the halves share nodes: concatenating would not pass)
    eg3d_host_free_graph3d(&g0), eg3d_host_free_graph3d(&g1), eg3d_host_free_graph3d(&gt), eg3d_host_free_graph3d(&want);
    eg3d_host_replay_state_destroy(top);
  }
  if (eg3d_host_replay_state_merge_graph(nullptr, nullptr, 0) != -1) bad |= 65536;
  eg3d_host_replay_state_destroy(by_cloud), eg3d_host_replay_state_destroy(by_graph);
  eg3d_host_replay_state_destroy(halves[0]), eg3d_host_replay_state_destroy(halves[1]);
  eg3d_synth_destroy(syn);
  printf("replay_merge_check %d\n", bad);
  return bad ? 1 : 0;
}
