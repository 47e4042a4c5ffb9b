// coordinate_system_transform — the reference's fourth tool (src/coordinate_system_transform/) on this library: an OpenMVG
// JSON reconstruction brought into the frame of known camera centres.
//
//   coordinate_system_transform [--host] input.json camera_poses.txt output.json
//
//   camera_poses.txt   one "x y z" triple per camera of input.json, in camera order (the triple of a camera without a
//                      pose is read and ignored)
//   --host             transform the points with the host statement (include/eg3d_host_transform.h): no GPU. Without it
//                      the points go through K16 on device 0 (include/eg3d_transform.h); a machine without a device is
//                      told to pass --host, nothing falls back silently.
//
// The fit (FP64, include/eg3d_host_transform.h) and the camera update always run on the host: tens of cameras. Both
// routes write the same bytes. Prints what the reference prints: the "Ignoring camera" lines, "T:" and the matrix, and
// the mean camera position error before and after (its divisor is ALL cameras: DESIGN.md 3, Q16).
// Build (tests/cbuild.py):
//   g++ -std=c++17 -I include examples/coordinate_system_transform.cpp -Ledgegraph3d_amd -leg3d -leg3d_host ...
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eg3d_host_transform.h"
#include "eg3d_transform.h"

namespace {

// a context on the JSON's cameras: one short polyline per view, no fundamental matrix (the transform reads neither)
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

// `cout << Matrix4d`: 6 significant digits, every coefficient right-aligned to the widest, one space between columns
void print_matrix(const double* T) {
  std::string text[16];
  size_t width = 0;
  for (int k = 0; k < 16; k++) {
    std::ostringstream os;
    os << T[k];
    text[k] = os.str();
    width = std::max(width, text[k].size());
  }
  for (int r = 0; r < 4; r++) {
    for (int c = 0; c < 4; c++) std::cout << (c ? " " : "") << std::string(width - text[4 * r + c].size(), ' ') << text[4 * r + c];
    std::cout << "\n";
  }
}

const char* why(int rc) {
  switch (rc) {
    case EG3D_TRANSFORM_ERR_FEW: return "fewer than 3 cameras with a pose";
    case EG3D_TRANSFORM_ERR_DEGENERATE: return "all camera centres of the reconstruction are equal";
    case EG3D_TRANSFORM_ERR_NONFINITE: return "a camera centre is not finite";
    case EG3D_TRANSFORM_ERR_FILE: return "the poses file cannot be opened";
    case EG3D_TRANSFORM_ERR_SHORT: return "the poses file holds fewer than three numbers per camera";
    default: return "bad arguments";
  }
}

float position_error(const eg3d_sfm* sfm, const std::vector<double>& target) {
  const int V = eg3d_sfm_n_views(sfm);
  std::vector<double> c64((size_t)V * 3);
  std::vector<uint8_t> null_mask((size_t)V);
  eg3d_sfm_camera_centres(sfm, c64.data(), null_mask.data());
  std::vector<float> c32(c64.begin(), c64.end());  // (the centres ARE floats: widened and narrowed exactly)
  float e = 0;
  eg3d_host_camera_errors(V, c32.data(), null_mask.data(), target.data(), &e);
  return e;
}

}  // namespace

int main(int argc, char** argv) {
  bool on_host = false;
  std::vector<const char*> rest;
  for (int a = 1; a < argc; a++) {
    if (std::strcmp(argv[a], "--host") == 0)
      on_host = true;
    else
      rest.push_back(argv[a]);
  }
  if (rest.size() != 3) {
    std::fprintf(stderr,
                 "Invalid input.\n\nCorrect format is:\n\n%s [--host] input.json camera_poses.txt output.json\n"
                 "\tinput.json : input structure from motion data in JSON format\n"
                 "\tcamera_poses.txt : target camera centres, one x y z triple per camera\n"
                 "\toutput.json : the transformed structure from motion data\n\n"
                 "Optional parameters:\n\n\t--host : transform the points on the host instead of the GPU\n\n",
                 argv[0]);
    return 1;
  }
  eg3d_sfm* sfm = eg3d_sfm_read_json(rest[0]);
  if (!sfm) {
    std::fprintf(stderr, "coordinate_system_transform: cannot read %s\n", rest[0]);
    return 1;
  }
  const int V = eg3d_sfm_n_views(sfm);
  const uint64_t n = eg3d_sfm_n_points(sfm);
  int rc = 0;
  eg3d_ctx* ctx = nullptr;
  do {
    std::vector<double> target((size_t)V * 3), centres((size_t)V * 3), T(16);
    std::vector<uint8_t> null_mask((size_t)V);
    if ((rc = eg3d_host_read_camera_poses(rest[1], V, target.data())) != 0) {
      std::fprintf(stderr, "coordinate_system_transform: %s: %s (%d cameras)\n", rest[1], why(rc), V);
      break;
    }
    std::cout << "Transforming coordinate system to adapt it to real camera poses..." << std::endl;
    eg3d_sfm_camera_centres(sfm, centres.data(), null_mask.data());
    for (int v = 0; v < V; v++)
      if (null_mask[(size_t)v]) std::cout << "Ignoring camera " << v << " in computing the Umeyama transformation" << std::endl;
    eg3d_similarity_stats fit;
    fit.struct_size = sizeof(fit);
    if ((rc = eg3d_host_similarity_fit(V, centres.data(), target.data(), null_mask.data(), T.data(), &fit)) != 0) {
      std::fprintf(stderr, "coordinate_system_transform: no fit: %s\n", why(rc));
      break;
    }
    if (fit.rank_deficient) std::fprintf(stderr, "coordinate_system_transform: the camera centres lie on a line: the rotation about it is arbitrary\n");
    std::cout << "T:" << std::endl;
    print_matrix(T.data());
    std::cout << "Camera position errors before: " << position_error(sfm, target) << std::endl;
    if (!on_host && eg3d_device_count() < 1) {
      std::fprintf(stderr, "coordinate_system_transform: no HIP device; pass --host to transform the points on the host\n");
      rc = 1;
      break;
    }
    if ((rc = eg3d_sfm_apply_transform(sfm, T.data(), on_host ? EG3D_SFM_TRANSFORM_CAMERAS | EG3D_SFM_TRANSFORM_POINTS
                                                              : EG3D_SFM_TRANSFORM_CAMERAS)) != 0) {
      std::fprintf(stderr, "coordinate_system_transform: the transform was refused (%d)\n", rc);
      break;
    }
    if (!on_host) {
      std::vector<float> X(3 * (size_t)n);
      eg3d_transform_stats st;
      st.struct_size = sizeof(st);
      if ((rc = make_context(sfm, &ctx)) != EG3D_OK ||
          (rc = eg3d_transform_points(ctx, T.data(), eg3d_sfm_points(sfm), n, X.data(), &st)) != EG3D_OK) {
        std::fprintf(stderr, "coordinate_system_transform: %s\n", eg3d_last_error());
        break;
      }
      if (n) eg3d_sfm_set_point_coords(sfm, X.data());
    }
    std::cout << "Camera position errors after: " << position_error(sfm, target) << std::endl;
    const int wr = eg3d_sfm_write_json(sfm, rest[0], rest[2]);
    if (wr == -2) std::fprintf(stderr, "coordinate_system_transform: a coordinate is not finite: %s is not a valid file\n", rest[2]);
    if (wr != 0) {
      if (wr != -2) std::fprintf(stderr, "coordinate_system_transform: cannot write %s\n", rest[2]);
      rc = 1;
      break;
    }
    std::printf("wrote %s (%d cameras, %llu points, scale %g, transformed on the %s)\n", rest[2], V, (unsigned long long)n, fit.scale,
                on_host ? "host" : "device");
  } while (false);
  if (ctx) eg3d_destroy(ctx);
  eg3d_sfm_destroy(sfm);
  return rc ? 1 : 0;
}
