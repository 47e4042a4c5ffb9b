// PLGMatchesManager::set_accumulate (include/eg3d_refapi.hpp) without a GPU: chains fed in two replay_chains calls with
// accumulation on must leave the graph of one call with all of them; with the default setting the second call replaces.
// Also the program the host state is run through under -fsanitize=address,undefined (create / add x n / graph / destroy).
#include <cstdio>
#include <cstring>
#include <vector>

#include "eg3d_host.h"
#include "eg3d_host_accumulate.h"
#include "eg3d_refapi.hpp"

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

int main() {
  using namespace eg3d_ref;
  typedef std::vector<std::vector<new_3dpoint_plgp_matches>> Chains;
  typedef std::vector<std::array<uint32_t, 3>> Keys;
  eg3d_synth_config cfg;
  eg3d_synth_default_config(&cfg, 0);
  eg3d_synth* syn = eg3d_synth_create(&cfg);
  const eg3d_scene& sc = *eg3d_synth_scene(syn);
  uint32_t pl = 0;  // view 0's first polyline with three segments
  while (sc.pl_vtx_off[pl + 1] - sc.pl_vtx_off[pl] < 4) pl++;
  auto pt = [&](float x, float y, float z, uint32_t seg) {
    new_3dpoint_plgp_matches p;
    std::get<0>(p) = vec3{x, y, z};
    const float* v = sc.vtx_xy + 2 * (sc.pl_vtx_off[pl] + seg);
    std::get<1>(p).push_back(PolyLineGraph2D::plg_point{pl, {seg, {v[0], v[1]}}});
    std::get<2>(p).push_back(0);
    return p;
  };
  // the second call repeats a node, a connection (in the other orientation) and an interval's start segment of the first
  const Chains c1 = {{pt(1, 2, 3, 0), pt(4, 5, 6, 1)}, {pt(7, 8, 9, 2), pt(1, 2, 3, 1)}};
  const Chains c2 = {{pt(4, 5, 6, 0), pt(1, 2, 3, 2), pt(9, 9, 9, 1)}, {pt(7, 8, 9, 0)}};
  const Keys k1 = {{0, 0, 0}, {1, 0, 0}}, k2 = {{2, 0, 0}, {3, 0, 0}};
  Chains all = c1;
  all.insert(all.end(), c2.begin(), c2.end());
  Keys kall = k1;
  kall.insert(kall.end(), k2.begin(), k2.end());
  int bad = 0;
  PLGMatchesManager one, acc, def, only2;
  if (one.replay_chains(sc, all, kall) != 0) bad |= 1;
  acc.set_accumulate(true);
  if (acc.replay_chains(sc, c1, k1) != 0) bad |= 2;
  if (acc.get_plg3d().n_polylines != 2) bad |= 4;
  if (acc.replay_chains(sc, c2, k2) != 0) bad |= 8;
  if (!same(acc.get_plg3d(), one.get_plg3d())) bad |= 16;
  if (one.get_plg3d().n_polylines != 3 || one.get_plg3d().n_nodes != 4) bad |= 32;
  // the default: the second call replaces
  if (def.replay_chains(sc, c1, k1) != 0 || def.replay_chains(sc, c2, k2) != 0) bad |= 64;
  if (only2.replay_chains(sc, c2, k2) != 0) bad |= 64;
  if (!same(def.get_plg3d(), only2.get_plg3d()) || same(def.get_plg3d(), one.get_plg3d())) bad |= 128;
  // switching accumulation off drops the state: the next replay replaces
  acc.set_accumulate(false);
  if (acc.replay_chains(sc, c2, k2) != 0 || !same(acc.get_plg3d(), only2.get_plg3d())) bad |= 256;

  // the host state by hand: create / add x n / graph / destroy, an empty cloud and a refused one among them
  eg3d_replay_state* st = eg3d_host_replay_state_create(&sc);
  if (!st) bad |= 512;
  const float X[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 2, 3};
  const float* v0 = sc.vtx_xy + 2 * sc.pl_vtx_off[pl];
  const float xy[8] = {v0[0], v0[1], v0[2], v0[3], v0[4], v0[5], v0[2], v0[3]};
  const uint64_t off[5] = {0, 1, 2, 3, 4};
  const int32_t view[4] = {0, 0, 0, 0};
  const uint32_t pls[4] = {pl, pl, pl, pl}, seg[4] = {0, 1, 2, 1};
  for (int round = 0; round < 40 && st; round++) {  // (enough nodes for the table to grow several times)
    std::vector<float> Xr(X, X + 12);
    for (int q = 0; q < 12; q++) Xr[q] += 16.f * (float)(round / 2);
    const uint32_t key[16] = {(uint32_t)(2 * round), 0, 0, 0, (uint32_t)(2 * round), 0, 0, 1,
                              (uint32_t)(2 * round + 1), 0, 0, 0, (uint32_t)(2 * round + 1), 0, 0, 1};
    eg3d_edgepoints e;
    memset(&e, 0, sizeof(e));
    e.n_points = 4, e.n_obs = 4;
    e.X = Xr.data(), e.obs_off = const_cast<uint64_t*>(off), e.obs_view = const_cast<int32_t*>(view);
    e.obs_pl = const_cast<uint32_t*>(pls), e.obs_seg = const_cast<uint32_t*>(seg), e.obs_xy = const_cast<float*>(xy);
    e.key = const_cast<uint32_t*>(key);
    if (eg3d_host_replay_state_add(st, &e) != 0) bad |= 1024;
    eg3d_edgepoints none;
    memset(&none, 0, sizeof(none));
    if (eg3d_host_replay_state_add(st, &none) != 0) bad |= 2048;
    eg3d_edgepoints cut = e;  // its first point would continue the chain just added: refused
    uint32_t kc[16];
    memcpy(kc, key, sizeof(kc));
    kc[0] = kc[4] = (uint32_t)(2 * round + 1), kc[3] = 2, kc[7] = 3;
    cut.key = kc;
    if (eg3d_host_replay_state_add(st, &cut) != -1) bad |= 4096;
    eg3d_graph3d g;
    if (eg3d_host_replay_state_graph(st, &g) != 0) bad |= 8192;
    if (g.n_nodes != 3u * (uint64_t)(round / 2 + 1) || eg3d_host_replay_state_points(st) != 4u * (uint64_t)(round + 1)) bad |= 16384;
    eg3d_host_free_graph3d(&g);
  }
  eg3d_host_replay_state_destroy(st);
  eg3d_synth_destroy(syn);
  printf("accumulate_check %d\n", bad);
  return bad ? 1 : 0;
}
