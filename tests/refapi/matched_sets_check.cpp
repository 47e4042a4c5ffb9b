// GPU check of the matches-manager side of include/eg3d_refapi.hpp: synthetic config 0 is poured into the shim's types as in
// polymatch_check.cpp, pipeline 3 runs through plg_matching_from_refpoints_parallel(sfm, em, cm, plgmm), and then
//   M lines   plgmm.is_matched on the midpoint of every segment of every polyline:
//             "M view polyline segment x y matched start_seg end_seg" (coordinates as float bit patterns)
//   S/P/O     find_new_3d_points_from_compatible_polylines_expandallviews_parallel(sfm, em, set, plgmm) for the set of every
//             3-D curve: "S set n_points", per point "P x y z n_obs", per observation "O view polyline segment x y"
// for tests/test_gpu_matched_sets.py to compare with the host probe and with the C ABI's matched call.
#include <cstdio>
#include <cstring>

#include "eg3d_host.h"
#include "eg3d_refapi.hpp"

using namespace eg3d_ref;

static unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main() {
  eg3d_synth_config cfg;
  eg3d_synth_default_config(&cfg, 0);
  eg3d_synth* syn = eg3d_synth_create(&cfg);
  const eg3d_scene* sc = eg3d_synth_scene(syn);
  const eg3d_seeds* sd = eg3d_synth_seeds(syn);
  const int V = sc->n_views;

  SfMData sfm;
  sfm.numCameras_ = V;
  sfm.numPoints_ = (int)sd->n_seeds;
  sfm.imageWidth_ = sc->width;
  sfm.imageHeight_ = sc->height;
  sfm.camerasList_.resize(V);
  for (int v = 0; v < V; v++)
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) sfm.camerasList_[v].cameraMatrix[r][c] = sc->cam_P[v * 16 + r * 4 + c];
  sfm.points_.assign(sd->n_seeds, vec3{0, 0, 0});
  sfm.camViewingPointN_.resize(sd->n_seeds);
  sfm.point2DoncamViewingPoint_.resize(sd->n_seeds);
  for (uint32_t i = 0; i < sd->n_seeds; i++)
    for (uint32_t j = sd->trk_off[i]; j < sd->trk_off[i + 1]; j++) {
      sfm.camViewingPointN_[i].push_back(sd->trk_view[j]);
      sfm.point2DoncamViewingPoint_[i].push_back(vec2{sd->trk_xy[2 * j], sd->trk_xy[2 * j + 1]});
    }
  FundamentalMatrices F(V, std::vector<std::array<double, 9>>(V));
  for (int i = 0; i < V; i++)
    for (int j = 0; j < V; j++)
      for (int k = 0; k < 9; k++) F[i][j][k] = sc->F_valid[i * V + j] ? sc->F[((size_t)i * V + j) * 9 + k] : 0.0;
  std::vector<PolyLineGraph2D> plgs(V);
  for (int v = 0; v < V; v++) {
    PolyLineGraph2D& g = plgs[v];
    for (uint32_t p = sc->view_pl_off[v]; p < sc->view_pl_off[v + 1]; p++) {
      PolyLineGraph2D::polyline pl;
      const uint32_t a = sc->pl_vtx_off[p], b = sc->pl_vtx_off[p + 1];
      for (uint32_t k = a; k < b; k++) pl.polyline_coords.push_back(vec2{sc->vtx_xy[2 * k], sc->vtx_xy[2 * k + 1]});
      pl.start = sc->pl_start[p];
      pl.end = sc->pl_end[p];
      const unsigned long hi = pl.start > pl.end ? pl.start : pl.end;
      if (g.nodes_coords.size() <= hi) g.nodes_coords.resize(hi + 1, vec2{-1, -1});
      if (b - a > 1 && sc->pl_valid[p]) {
        g.nodes_coords[pl.start] = pl.polyline_coords.front();
        g.nodes_coords[pl.end] = pl.polyline_coords.back();
      }
      g.polylines.push_back(std::move(pl));
    }
  }

  PLGEdgeManager em(sfm, F, plgs, 0);
  if (em.last_status() != EG3D_OK) {
    std::printf("FAIL create: %s\n", eg3d_last_error());
    return 1;
  }
  PLGPCM3ViewsPLGFollowing cm(em);
  PLGMatchesManager plgmm;
  PolyLineGraph2D::pl_interval pli;
  // a manager that has replayed nothing holds nothing
  if (plgmm.is_matched(0, 0, PolyLineGraph2D::pl_point{0, vec2{0, 0}}, pli)) return 2;
  const auto cloud3 = plg_matching_from_refpoints_parallel(sfm, &em, &cm, plgmm);
  std::printf("R %zu\n", cloud3.size());

  const eg3d_scene& es = em.scene();
  for (int v = 0; v < V; v++)
    for (uint32_t p = es.view_pl_off[v]; p < es.view_pl_off[v + 1]; p++) {
      const uint32_t a = es.pl_vtx_off[p], b = es.pl_vtx_off[p + 1];
      if (!es.pl_valid[p] || b - a < 2) continue;
      for (uint32_t k = a; k + 1 < b; k++) {
        const float x = (es.vtx_xy[2 * k] + es.vtx_xy[2 * k + 2]) * 0.5f, y = (es.vtx_xy[2 * k + 1] + es.vtx_xy[2 * k + 3]) * 0.5f;
        const PolyLineGraph2D::plg_point q{p - es.view_pl_off[v], {k - a, vec2{x, y}}};
        const bool m = plgmm.is_matched(v, q, pli);
        std::printf("M %d %u %u %08x %08x %d %lu %lu\n", v, p - es.view_pl_off[v], k - a, bits(x), bits(y), m ? 1 : 0,
                    m ? pli.start.segment_index : 0ul, m ? pli.end.segment_index : 0ul);
      }
    }

  const uint32_t* curve = eg3d_synth_polyline_curve(syn);
  const int n_curves = eg3d_synth_n_curves(syn);
  for (int c = 0; c < n_curves; c++) {
    std::vector<std::set<unsigned long>> compat(V);
    for (int v = 0; v < V; v++)
      for (uint32_t p = sc->view_pl_off[v]; p < sc->view_pl_off[v + 1]; p++)
        if (curve[p] == (uint32_t)c && sc->pl_valid[p] && sc->pl_vtx_off[p + 1] - sc->pl_vtx_off[p] >= 2)
          compat[v].insert(p - sc->view_pl_off[v]);
    const auto pts = find_new_3d_points_from_compatible_polylines_expandallviews_parallel(sfm, &em, compat, plgmm);
    std::printf("S %d %zu\n", c, pts.size());
    for (const auto& pt : pts) {
      const vec3& X = std::get<0>(pt);
      const auto& obs = std::get<1>(pt);
      const auto& views = std::get<2>(pt);
      std::printf("P %08x %08x %08x %zu\n", bits(X.x), bits(X.y), bits(X.z), obs.size());
      for (size_t j = 0; j < obs.size(); j++)
        std::printf("O %d %lu %lu %08x %08x\n", views[j], obs[j].polyline_id, obs[j].plp.segment_index, bits(obs[j].plp.coords.x),
                    bits(obs[j].plp.coords.y));
    }
  }
  eg3d_synth_destroy(syn);
  return 0;
}
