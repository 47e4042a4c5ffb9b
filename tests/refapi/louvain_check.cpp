// GPU check of pipeline 1's community detection through include/eg3d_refapi.hpp: a synthetic scene is poured into the shim's
// types as in simgraph_check.cpp; compute_communities (the reference's shape) writes the compatibility graph to argv[2] and
// the community ids to argv[3] and returns them. Printed for tests/test_gpu_louvain.py: the returned ids on one line, then
// the ids of SimilarityGraph::communities with max_phases = 1 on the next.
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
  const std::vector<long> ids = compute_communities(graph, argv[2], argv[3]);
  if (ids.size() != graph.polyline_matches_vector.size()) return 5;
  for (long id : ids) std::printf("%ld ", id);
  std::printf("\n");
  eg3d_louvain_params one;
  std::memset(&one, 0, sizeof(one));
  one.struct_size = (uint32_t)sizeof(one);
  one.max_phases = 1;
  eg3d_louvain_stats st;
  st.struct_size = (uint32_t)sizeof(st);
  for (long id : graph.communities(&one, &st)) std::printf("%ld ", id);
  std::printf("\n%u %u\n", st.n_phases, st.n_communities);
  eg3d_synth_destroy(syn);
  return 0;
}
