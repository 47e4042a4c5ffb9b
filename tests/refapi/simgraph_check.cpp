// GPU check of the pipeline 1 functions of include/eg3d_refapi.hpp: a synthetic scene is poured into the shim's types as in
// polymatch_check.cpp; polyline_matching_similarity_graph_before_communities writes its graph to argv[2]; the community ids
// of argv[3] go through compute_polyline_matches_from_nodes_component_ids. Printed for tests/test_gpu_simgraph.py: one line
// per point with its close polylines as view:id, one line per (view, polyline) with its close reference points, a line
// "sets", then one line per (match, view) with the polyline ids.
#include <cstdio>
#include <cstring>

#include "eg3d_host.h"
#include "eg3d_refapi.hpp"

using namespace eg3d_ref;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int cfg_index = argc > 1 ? atoi(argv[1]) : 1;
  eg3d_synth_config cfg;
  eg3d_synth_default_config(&cfg, cfg_index);
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
  // polyline graphs: node ids of the flat scene become node coordinates = the end vertices
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
  const auto graph = polyline_matching_similarity_graph_before_communities(sfm, &em);
  if (graph.write_to_file(argv[2]) != EG3D_OK) return 3;
  for (const auto& point : graph.close_polylines) {
    for (int v = 0; v < V; v++)
      for (unsigned long id : point[v]) std::printf("%d:%lu ", v, id);
    std::printf("\n");
  }
  for (const auto& view : graph.close_refpoints)
    for (const auto& row : view) {
      for (unsigned long r : row) std::printf("%lu ", r);
      std::printf("\n");
    }
  int64_t* ids = nullptr;
  uint64_t n_ids = 0;
  if (eg3d_host_read_communities(argv[3], &ids, &n_ids) != EG3D_OK) return 4;
  const std::vector<long> component_ids(ids, ids + n_ids);
  eg3d_host_free(ids);
  if (component_ids.size() != graph.polyline_matches_vector.size()) return 5;
  std::printf("sets\n");
  for (const auto& match : compute_polyline_matches_from_nodes_component_ids(graph.polyline_matches_vector, V, component_ids))
    for (const auto& per_view : match) {
      for (unsigned long id : per_view) std::printf("%lu ", id);
      std::printf("\n");
    }
  eg3d_synth_destroy(syn);
  return 0;
}
