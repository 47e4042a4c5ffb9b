// GPU check of compute_3d_point_coords of include/eg3d_refapi.hpp: the seed tracks of a synthetic scene through the batched
// overload (no edge manager registered: a private context built from the cameras alone) and the first tracks once more
// through the reference's one-point signature. One line per track for tests/test_gpu_triangulate_example.py: valid, flags,
// the three coordinates as hexadecimal bit patterns; then "single <n>" and n lines valid + bit patterns.
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

int main(int argc, char** argv) {
  const int cfg_index = argc > 1 ? atoi(argv[1]) : 1;
  eg3d_synth_config cfg;
  eg3d_synth_default_config(&cfg, cfg_index);
  eg3d_synth* syn = eg3d_synth_create(&cfg);
  const eg3d_scene* sc = eg3d_synth_scene(syn);
  const eg3d_seeds* sd = eg3d_synth_seeds(syn);
  const int V = sc->n_views;
  SfMData sfm;
  sfm.numCameras_ = V;
  sfm.imageWidth_ = sc->width;
  sfm.imageHeight_ = sc->height;
  sfm.camerasList_.resize(V);
  for (int v = 0; v < V; v++)
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) sfm.camerasList_[v].cameraMatrix[r][c] = sc->cam_P[v * 16 + r * 4 + c];
  std::vector<std::vector<vec2>> coords(sd->n_seeds);
  std::vector<std::vector<int>> ids(sd->n_seeds);
  for (uint32_t i = 0; i < sd->n_seeds; i++)
    for (uint32_t j = sd->trk_off[i]; j < sd->trk_off[i + 1]; j++) {
      ids[i].push_back(sd->trk_view[j]);
      coords[i].push_back(vec2{sd->trk_xy[2 * j], sd->trk_xy[2 * j + 1]});
    }
  coords.push_back(std::vector<vec2>(coords[0].begin(), coords[0].begin() + 1));  // a short track at the end
  ids.push_back(std::vector<int>(ids[0].begin(), ids[0].begin() + 1));
  std::vector<vec3> pts;
  std::vector<bool> valid;
  std::vector<uint8_t> flags;
  try {
    compute_3d_point_coords(sfm, coords, ids, pts, valid, &flags);
    for (size_t i = 0; i < pts.size(); i++)
      std::printf("%d %u %08x %08x %08x\n", valid[i] ? 1 : 0, (unsigned)flags[i], bits(pts[i].x), bits(pts[i].y), bits(pts[i].z));
    const size_t n1 = coords.size() < 3 ? coords.size() : 3;
    std::printf("single %zu\n", n1 + 1);
    for (size_t k = 0; k <= n1; k++) {
      const size_t i = k < n1 ? k : coords.size() - 1;  // (the short one last)
      vec3 p{7.f, 7.f, 7.f};
      bool ok = true;
      compute_3d_point_coords(sfm, coords[i], ids[i], p, ok);
      std::printf("%d %08x %08x %08x\n", ok ? 1 : 0, bits(p.x), bits(p.y), bits(p.z));
    }
  } catch (const Eg3dError& e) {
    std::printf("FAIL %s\n", e.what());
    return 1;
  }
  eg3d_synth_destroy(syn);
  return 0;
}
