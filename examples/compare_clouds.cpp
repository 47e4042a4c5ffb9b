// compare_clouds — two point clouds compared by nearest distances (K18, include/eg3d/nearest.hpp): what the reference's
// coordinate_system_transform prepares (example/dtu006/README.md: clouds of one object are compared in one coordinate system).
//
//   compare_clouds A B --max-dist D [--cell C] [--threshold T]... [--host]
//
//   A, B          each a PLY file (ASCII or binary little-endian; the `element vertex` is taken) or an OpenMVG JSON, whose
//                 `structure` is taken. A is the cloud under test, B the reference.
//   --max-dist D  the reach of the search: a point with nothing within D has no distance
//   --cell C      the grid's edge (default D; must be >= D)
//   --threshold T up to 8: the fraction of points nearer than T is printed
//   --host        compute with the host statement (include/eg3d/host_nearest.hpp): no GPU. Without it both directions run
//                 on device 0; a machine without a device is told to pass --host, nothing falls back silently.
//
// Prints accuracy (A -> B) and completeness (B -> A): points, points within reach, mean and median distance, the fraction
// below each threshold. Both routes print identical text: the figures are exact.
// Build (tests/cbuild.py):
//   g++ -std=c++17 -I include examples/compare_clouds.cpp -Ledgegraph3d_amd -leg3d -leg3d_host ...
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "eg3d/nearest.hpp"
#include "eg3d_host.h"

namespace {

bool ends_with(const std::string& s, const char* tail) {
  const size_t n = std::strlen(tail);
  return s.size() >= n && s.compare(s.size() - n, n, tail) == 0;
}

bool load(const char* path, std::vector<float>* X) {
  if (ends_with(path, ".json")) {
    eg3d_sfm* sfm = eg3d_sfm_read_json(path);
    if (!sfm) {
      std::fprintf(stderr, "compare_clouds: cannot read %s\n", path);
      return false;
    }
    const uint64_t n = eg3d_sfm_n_points(sfm);
    if (n) X->assign(eg3d_sfm_points(sfm), eg3d_sfm_points(sfm) + 3 * n);
    eg3d_sfm_destroy(sfm);
    return true;
  }
  float* p = nullptr;
  uint64_t n = 0;
  if (eg3d_host_read_ply_points(path, &p, &n) != 0) {
    std::fprintf(stderr, "compare_clouds: %s: %s\n", path, eg3d_host_nearest_last_error());
    return false;
  }
  X->assign(p, p + 3 * n);
  eg3d_host_free_points(p);
  return true;
}

// a context for clouds that come without a scene: two views, one short polyline each, no fundamental matrix
int make_context(eg3d_ctx** ctx) {
  const int V = 2;
  std::vector<float> P = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0};
  std::vector<double> F((size_t)V * V * 9, 0.0);
  std::vector<uint8_t> Fv((size_t)V * V, 0), valid((size_t)V, 1);
  std::vector<uint32_t> vpo = {0, 1, 2}, pvo = {0, 2, 4}, start = {0, 2}, end = {1, 3};
  std::vector<float> vtx = {0.5f, 0.5f, 2.5f, 0.5f, 0.5f, 0.5f, 2.5f, 0.5f};
  eg3d_scene sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.n_views = V;
  sc.width = sc.height = 8;
  sc.cam_P = P.data();
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

void print_side(const char* name, const eg3d_nearest_stats& s, float max_dist) {
  const uint64_t used = s.n_queries - s.n_dropped - s.n_nonfinite;
  std::printf("%s: %llu points (%llu not finite), %llu within %g", name, (unsigned long long)s.n_queries, (unsigned long long)s.n_nonfinite,
              (unsigned long long)s.n_within, (double)max_dist);
  if (s.n_within) {
    const double mean = (double)s.sum_q32 * (double)max_dist / 4294967296.0 / (double)s.n_within;
    std::printf(", mean %.9g, median %.9g", mean, std::sqrt((double)s.median_d2));
  }
  std::printf("\n");
  for (uint32_t k = 0; k < s.n_thresholds; k++)
    std::printf("  below %g: %llu (%.4f%%)\n", (double)s.thresholds[k], (unsigned long long)s.n_below[k],
                used ? 100.0 * (double)s.n_below[k] / (double)used : 0.0);
}

}  // namespace

int main(int argc, char** argv) {
  bool on_host = false;
  float max_dist = 0.f, cell = 0.f;
  std::vector<float> th;
  std::vector<const char*> rest;
  for (int a = 1; a < argc; a++) {
    if (std::strcmp(argv[a], "--host") == 0)
      on_host = true;
    else if (std::strcmp(argv[a], "--max-dist") == 0 && a + 1 < argc)
      max_dist = std::strtof(argv[++a], nullptr);
    else if (std::strcmp(argv[a], "--cell") == 0 && a + 1 < argc)
      cell = std::strtof(argv[++a], nullptr);
    else if (std::strcmp(argv[a], "--threshold") == 0 && a + 1 < argc)
      th.push_back(std::strtof(argv[++a], nullptr));
    else
      rest.push_back(argv[a]);
  }
  if (rest.size() != 2 || !(max_dist > 0.f) || th.size() > EG3D_NEAREST_MAX_THRESHOLDS) {
    std::fprintf(stderr, "usage: %s A B --max-dist D [--cell C] [--threshold T]... [--host]\n\tA, B : PLY files or OpenMVG JSON files\n"
                         "\t--max-dist D : the reach of the search (> 0)\n\t--cell C : the grid's edge (default D)\n"
                         "\t--threshold T : up to 8, each in (0, D]\n\t--host : compute on the host instead of the GPU\n", argv[0]);
    return 1;
  }
  if (!(cell > 0.f)) cell = max_dist;
  std::vector<float> A, B;
  if (!load(rest[0], &A) || !load(rest[1], &B)) return 1;
  const uint64_t na = A.size() / 3, nb = B.size() / 3;
  eg3d_nearest_stats acc, comp;
  std::memset(&acc, 0, sizeof(acc));
  acc.struct_size = sizeof(acc);
  acc.n_thresholds = (uint32_t)th.size();
  for (size_t k = 0; k < th.size(); k++) acc.thresholds[k] = th[k];
  comp = acc;
  int rc = 0;
  if (on_host) {
    if ((rc = eg3d_host_cloud_nearest(B.data(), nb, nullptr, A.data(), na, nullptr, cell, max_dist, nullptr, nullptr, &acc)) != 0 ||
        (rc = eg3d_host_cloud_nearest(A.data(), na, nullptr, B.data(), nb, nullptr, cell, max_dist, nullptr, nullptr, &comp)) != 0) {
      std::fprintf(stderr, "compare_clouds: %s\n", eg3d_host_nearest_last_error());
      return 1;
    }
  } else {
    if (eg3d_device_count() < 1) {
      std::fprintf(stderr, "compare_clouds: no HIP device; pass --host to compare on the host\n");
      return 1;
    }
    eg3d_ctx* ctx = nullptr;
    eg3d_cloud_index *ia = nullptr, *ib = nullptr;
    if ((rc = make_context(&ctx)) != EG3D_OK || (rc = eg3d_cloud_index_build(ctx, B.data(), nb, nullptr, cell, &ib, nullptr)) != EG3D_OK ||
        (rc = eg3d_cloud_nearest_points(ctx, A.data(), na, nullptr, ib, max_dist, nullptr, nullptr, &acc)) != EG3D_OK ||
        (rc = eg3d_cloud_index_build(ctx, A.data(), na, nullptr, cell, &ia, nullptr)) != EG3D_OK ||
        (rc = eg3d_cloud_nearest_points(ctx, B.data(), nb, nullptr, ia, max_dist, nullptr, nullptr, &comp)) != EG3D_OK)
      std::fprintf(stderr, "compare_clouds: %s\n", eg3d_last_error());
    eg3d_cloud_index_free(ia);
    eg3d_cloud_index_free(ib);
    if (ctx) eg3d_destroy(ctx);
    if (rc) return 1;
  }
  print_side("accuracy (A -> B)", acc, max_dist);
  print_side("completeness (B -> A)", comp, max_dist);
  return 0;
}
