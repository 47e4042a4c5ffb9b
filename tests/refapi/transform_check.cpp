// transform_check.cpp — TEST-ONLY caller of include/eg3d_transform_coordinate_system.hpp (tests/
// test_coordinate_system_transform_tool.py): a PosedSfMData from a raw float32 file, update_sfmd_from_real_camera_positions
// on it — on the host, or with "device" as the fourth argument on a context's device —, the result back as raw float32.
//   transform_check in.bin poses.txt out.bin [device]
//   in.bin : V, n (as floats), then per camera focal, ppx, ppy, R[9], C[3], t[3], then X[3 n]
//   out.bin: per camera R[9], C[3], t[3], cameraMatrix[16], then X[3 n]
#include <cstdio>
#include <cstring>
#include <vector>

#include "eg3d_transform_coordinate_system.hpp"

static eg3d_ctx* tiny_context() {  // three views, one two-vertex polyline each (as examples/json_to_ply.cpp): the transform reads none
  static float P[48];
  static double F[81] = {0};
  static uint8_t Fv[9] = {0}, valid[3] = {1, 1, 1};
  static uint32_t vpo[4] = {0, 1, 2, 3}, pvo[4] = {0, 2, 4, 6}, start[3] = {0, 2, 4}, end[3] = {1, 3, 5};
  static float vtx[12] = {0.5f, 0.5f, 2.5f, 0.5f, 0.5f, 0.5f, 2.5f, 0.5f, 0.5f, 0.5f, 2.5f, 0.5f};
  for (int v = 0; v < 3; v++) {
    const float one[16] = {1, 0, 0, (float)v, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0};
    std::memcpy(P + 16 * v, one, sizeof(one));
  }
  eg3d_scene sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.n_views = 3;
  sc.width = sc.height = 8;
  sc.cam_P = P;
  sc.F = F;
  sc.F_valid = Fv;
  sc.view_pl_off = vpo;
  sc.pl_vtx_off = pvo;
  sc.vtx_xy = vtx;
  sc.pl_start = start;
  sc.pl_end = end;
  sc.pl_valid = valid;
  eg3d_ctx* ctx = nullptr;
  return eg3d_create(&sc, 0, &ctx) == EG3D_OK ? ctx : nullptr;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<float> in;
  float buf[256];
  for (size_t k; (k = std::fread(buf, sizeof(float), 256, f)) > 0;) in.insert(in.end(), buf, buf + k);
  std::fclose(f);
  const int V = (int)in[0], n = (int)in[1];
  if (in.size() != 2 + 18 * (size_t)V + 3 * (size_t)n) return 2;
  eg3d_ref::PosedSfMData s;
  s.numCameras_ = V;
  s.numPoints_ = n;
  s.camerasList_.resize((size_t)V);
  s.poses_.resize((size_t)V);
  const float* p = in.data() + 2;
  for (int v = 0; v < V; v++, p += 18) {
    eg3d_ref::CameraPose& c = s.poses_[(size_t)v];
    c.intrinsics[0][0] = c.intrinsics[1][1] = p[0];
    c.intrinsics[0][2] = p[1];
    c.intrinsics[1][2] = p[2];
    c.intrinsics[2][2] = 1.0f;
    std::memcpy(c.rotation, p + 3, sizeof(float) * 9);
    std::memcpy(c.center, p + 12, sizeof(float) * 3);
    std::memcpy(c.translation, p + 15, sizeof(float) * 3);
    std::memset(s.camerasList_[(size_t)v].cameraMatrix, 0, sizeof(float) * 16);
  }
  for (int i = 0; i < n; i++, p += 3) s.points_.push_back({p[0], p[1], p[2]});
  eg3d_ctx* ctx = nullptr;
  try {
    if (argc > 4 && std::strcmp(argv[4], "device") == 0) {
      ctx = tiny_context();
      if (!ctx) {
        std::fprintf(stderr, "no context: %s\n", eg3d_last_error());
        return 3;
      }
      eg3d_ref::update_sfmd_from_real_camera_positions(ctx, s, argv[2]);
    } else {
      eg3d_ref::update_sfmd_from_real_camera_positions(s, argv[2]);
    }
  } catch (const eg3d_ref::Eg3dError& e) {
    std::fprintf(stderr, "Eg3dError %d: %s\n", e.status, e.what());
    if (ctx) eg3d_destroy(ctx);
    return 4;
  }
  if (ctx) eg3d_destroy(ctx);
  f = std::fopen(argv[3], "wb");
  if (!f) return 2;
  for (int v = 0; v < V; v++) {
    const eg3d_ref::CameraPose& c = s.poses_[(size_t)v];
    std::fwrite(c.rotation, sizeof(float), 9, f);
    std::fwrite(c.center, sizeof(float), 3, f);
    std::fwrite(c.translation, sizeof(float), 3, f);
    std::fwrite(s.camerasList_[(size_t)v].cameraMatrix, sizeof(float), 16, f);
  }
  for (int i = 0; i < n; i++) std::fwrite(&s.points_[(size_t)i].x, sizeof(float), 3, f);
  std::fclose(f);
  return 0;
}
