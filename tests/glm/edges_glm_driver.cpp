// edges_glm_driver.cpp — TEST-ONLY. Evaluates, with the header-only glm the reference vendors (0.9.6; given with -I on the
// command line, nothing of it is copied), the glm expression of the reference's 3-D distance_point_line_sq
// (utils/geometry/geometric_utilities.cpp:1003-1005 with vec6::direction / vec6::start, utils/datatypes.cpp:60-69):
//   d = (b - a) component by component;  dot(c, c) / dot(d, d)  with  c = glm::cross(d, a - p)
// so that csrc/eg3d_edges_core.h can be pinned bit for bit against the reference's own math library.
// I/O: raw little-endian float32 records on stdin: p (3), a (3), b (3) = 9 floats; on stdout: one float per record.
// Compiled with the reference's release flags (-O3 -funroll-loops, baseline x86-64: no FMA).
#include <stdio.h>

#include <glm/glm.hpp>

int main() {
  float in[9], out;
  while (fread(in, sizeof(float), 9, stdin) == 9) {
    const glm::vec3 p(in[0], in[1], in[2]);
    const glm::vec3 start(in[3], in[4], in[5]);
    const glm::vec3 direction(in[6] - in[3], in[7] - in[4], in[8] - in[5]);
    const glm::vec3 c = glm::cross(direction, start - p);
    out = glm::dot(c, c) / glm::dot(direction, direction);
    fwrite(&out, sizeof(float), 1, stdout);
  }
  return 0;
}
