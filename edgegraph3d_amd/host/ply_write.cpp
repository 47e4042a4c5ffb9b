// ply_write.cpp — eg3d_host_write_ply (include/eg3d_host_colour.h): the ASCII PLY point cloud of the reference's
// output_point_cloud / output_colored_point_cloud, with and without `inliers` (io/output/output_point_cloud.cpp:127-257),
// byte for byte: `ostream << float` is %g of the widened value at precision 6, and the newline after a point's line is
// left out when the point's INDEX is the last one, whether or not later points were dropped.
#include <cstdio>
#include <string>

#include "eg3d_host_colour.h"

extern "C" int eg3d_host_write_ply(const char* path, uint64_t n_points, const float* X, const uint8_t* rgb, const uint8_t* keep) {
  if (!path || (n_points && !X)) return -1;
  uint64_t count = 0;
  for (uint64_t i = 0; i < n_points; i++) count += (!keep || keep[i]) ? 1 : 0;
  FILE* f = fopen(path, "wb");
  if (!f) return -2;
  std::string text = "ply\nformat ascii 1.0\nelement vertex " + std::to_string(count) +
                     "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
                     "property uchar blue\nend_header\n";
  bool ok = true;
  char line[160];
  for (uint64_t i = 0; i < n_points && ok; i++) {
    if (keep && !keep[i]) continue;
    const int r = rgb ? rgb[3 * i] : 255, g = rgb ? rgb[3 * i + 1] : 255, b = rgb ? rgb[3 * i + 2] : 255;
    const int n = snprintf(line, sizeof(line), "%g %g %g %d %d %d", (double)X[3 * i], (double)X[3 * i + 1], (double)X[3 * i + 2], r, g, b);
    text.append(line, (size_t)n);
    if (i != n_points - 1) text.push_back('\n');
    if (text.size() >= (1u << 20)) {
      ok = fwrite(text.data(), 1, text.size(), f) == text.size();
      text.clear();
    }
  }
  if (ok && !text.empty()) ok = fwrite(text.data(), 1, text.size(), f) == text.size();
  if (fclose(f) != 0) ok = false;
  return ok ? 0 : -2;
}
