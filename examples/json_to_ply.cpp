// json_to_ply — the reference's third tool (src/utils/json_to_ply.cpp) on this library: an OpenMVG JSON structure as an
// ASCII PLY point cloud, white or coloured from the source images.
//
//   json_to_ply [-i original_images/] [--host] input.json output.ply
//
//   without -i   white points (output_point_cloud); no GPU is touched
//   -i DIR/      coloured points (output_colored_point_cloud): the image of view v is DIR/ + the base name of the view's
//                path in the JSON (no separator is added, as in the reference), a PNG (JPEG is not read). The colours are
//                computed on the device (K15, include/eg3d_colour.h) ...
//   --host       ... or, with this switch, by the host statement (include/eg3d_host_colour.h): no GPU
//
// Both routes write the same bytes. The device route needs a context, and a context needs a scene: the tool gives it the
// JSON's cameras and one two-vertex polyline per view, which the colouring never reads.
// Build (tests/cbuild.py):
//   g++ -std=c++17 -I include examples/json_to_ply.cpp -Ledgegraph3d_amd -leg3d -leg3d_host ...
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "eg3d_point_cloud.hpp"

namespace {

eg3d_ref::SfMData to_sfmd(const eg3d_sfm* sfm) {
  eg3d_ref::SfMData d;
  d.numCameras_ = eg3d_sfm_n_views(sfm);
  d.numPoints_ = (int)eg3d_sfm_n_points(sfm);
  eg3d_sfm_image_size(sfm, &d.imageWidth_, &d.imageHeight_);
  for (int v = 0; v < d.numCameras_; v++) d.camerasPaths_.push_back(eg3d_sfm_image_path(sfm, v));
  eg3d_seeds t;
  eg3d_sfm_seeds(sfm, &t);
  const float* X = eg3d_sfm_points(sfm);
  for (int i = 0; i < d.numPoints_; i++) {
    d.points_.push_back({X[3 * i], X[3 * i + 1], X[3 * i + 2]});
    std::vector<int> cams;
    std::vector<eg3d_ref::vec2> at;
    for (uint32_t k = t.trk_off[i]; k < t.trk_off[i + 1]; k++) {
      cams.push_back(t.trk_view[k]);
      at.push_back({t.trk_xy[2 * k], t.trk_xy[2 * k + 1]});
    }
    d.camViewingPointN_.push_back(cams);
    d.point2DoncamViewingPoint_.push_back(at);
  }
  return d;
}

// a context on the JSON's cameras: one short polyline per view, no fundamental matrix
int make_context(const eg3d_sfm* sfm, eg3d_ctx** ctx) {
  const int V = eg3d_sfm_n_views(sfm);
  int W = 0, H = 0;
  eg3d_sfm_image_size(sfm, &W, &H);
  std::vector<double> F((size_t)V * V * 9, 0.0);
  std::vector<uint8_t> Fv((size_t)V * V, 0), valid((size_t)V, 1);
  std::vector<uint32_t> vpo((size_t)V + 1), pvo((size_t)V + 1), start((size_t)V), end((size_t)V);
  std::vector<float> vtx;
  for (int v = 0; v <= V; v++) vpo[(size_t)v] = (uint32_t)v, pvo[(size_t)v] = 2u * (uint32_t)v;
  for (int v = 0; v < V; v++) {
    start[(size_t)v] = 2u * (uint32_t)v;
    end[(size_t)v] = 2u * (uint32_t)v + 1u;
    vtx.insert(vtx.end(), {0.5f, 0.5f, 2.5f, 0.5f});
  }
  eg3d_scene sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.n_views = V;
  sc.width = W > 0 ? W : 1;
  sc.height = H > 0 ? H : 1;
  sc.cam_P = eg3d_sfm_cam_P(sfm);
  sc.F = F.data();
  sc.F_valid = Fv.data();
  sc.view_pl_off = vpo.data();
  sc.pl_vtx_off = pvo.data();
  sc.vtx_xy = vtx.data();
  sc.pl_start = start.data();
  sc.pl_end = end.data();
  sc.pl_valid = valid.data();
  return eg3d_create(&sc, 0, ctx);
}

}  // namespace

int main(int argc, char** argv) {
  const char* images = nullptr;
  bool on_host = false;
  std::vector<const char*> rest;
  for (int a = 1; a < argc; a++) {
    if (std::strcmp(argv[a], "-i") == 0 && a + 1 < argc)
      images = argv[++a];
    else if (std::strcmp(argv[a], "--host") == 0)
      on_host = true;
    else
      rest.push_back(argv[a]);
  }
  if (rest.size() != 2) {
    std::fprintf(stderr,
                 "Invalid input.\n\nCorrect format is:\n\n%s [-i images/] [--host] input.json output.ply\n"
                 "\tinput.json : input structure from motion data in JSON format\n\toutput.ply : output point cloud in PLY format\n\n"
                 "Optional parameters:\n\n\t-i images/ : PNG images originally used to produce the provided structure from motion data. "
                 "If this argument is provided, json_to_ply will produce a colored point cloud\n"
                 "\t--host : compute the colours on the host instead of the GPU\n\n",
                 argv[0]);
    return 1;
  }
  std::printf("Input: %s\nOutput: %s\n", rest[0], rest[1]);
  eg3d_sfm* sfm = eg3d_sfm_read_json(rest[0]);
  if (!sfm) {
    std::fprintf(stderr, "json_to_ply: cannot read %s\n", rest[0]);
    return 1;
  }
  int rc = 0;
  eg3d_ctx* ctx = nullptr;
  try {
    const eg3d_ref::SfMData sfmd = to_sfmd(sfm);
    if (!images) {
      eg3d_ref::output_point_cloud(sfmd, rest[1]);
    } else if (on_host) {
      eg3d_ref::output_colored_point_cloud(sfmd, images, rest[1]);
    } else {
      if (make_context(sfm, &ctx) != EG3D_OK) throw eg3d_ref::Eg3dError(EG3D_ERR_HIP, std::string("no device context: ") + eg3d_last_error());
      eg3d_ref::output_colored_point_cloud(ctx, sfmd, images, rest[1]);
    }
    std::printf("wrote %s (%d points%s)\n", rest[1], sfmd.numPoints_, !images ? "" : on_host ? ", coloured on the host" : ", coloured on the device");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "json_to_ply: %s\n", e.what());
    rc = 1;
  }
  if (ctx) eg3d_destroy(ctx);
  eg3d_sfm_destroy(sfm);
  return rc;
}
