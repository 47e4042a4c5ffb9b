// edges_core_driver.cpp — TEST-ONLY. The host compilation of csrc/eg3d_edges_core.h's distance_point_line_sq behind the I/O
// of edges_glm_driver.cpp: 9 floats (p, a, b) per record on stdin, one float per record on stdout. Compiled with the host
// library's arithmetic flags (-O2 -ffp-contract=off -fno-fast-math).
#include <stdio.h>

#include "eg3d_edges_core.h"

int main() {
  float in[9], out;
  while (fread(in, sizeof(float), 9, stdin) == 9) {
    out = eg3d::edges::distance_point_line_sq(in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8]);
    fwrite(&out, sizeof(float), 1, stdout);
  }
  return 0;
}
