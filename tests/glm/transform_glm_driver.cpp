// transform_glm_driver.cpp — TEST-ONLY. Evaluates, with the header-only glm the reference vendors (0.9.6; given with -I
// on the command line, nothing of it is copied), the glm expressions of the reference's coordinate_system_transform
// (coordinate_system_transform/transform_coordinate_system.cpp:152-174), so that the host statement of
// include/eg3d_host_transform.h can be pinned bit for bit against the reference's own math library:
//   point    tmp = vec4(pt, 1) * M; (tmp[0] / tmp[3], tmp[1] / tmp[3], tmp[2] / tmp[3])
//   inverse  glm::inverse(M)
//   e        glm::inverse(M) * rt4x4(R, t)       (the layout of get_rt4x4, edge_graph_3d_utilities.cpp:565-571)
//   P        e * K4, K4 = the intrinsics in the top-left 3 x 3 of a zero mat4
// I/O: raw little-endian float32 records on stdin: M[4][4] as filled [i][j] (16), R[3][3] (9), t (3), focal, ppx, ppy (3),
// pt (3) = 34 floats; on stdout: the point (3), the inverse (16), e (16), P (16) = 51 floats, each matrix as read [i][j].
// Compiled with the reference's release flags (-O3 -funroll-loops, baseline x86-64: no FMA).
#include <stdio.h>

#include <glm/glm.hpp>

static void put(float* out, const glm::mat4& m) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) out[4 * i + j] = m[i][j];
}

int main() {
  float in[34], out[51];
  while (fread(in, sizeof(float), 34, stdin) == 34) {
    glm::mat4 M;
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) M[i][j] = in[4 * i + j];
    glm::mat3 r;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) r[i][j] = in[16 + 3 * i + j];
    const glm::vec3 t(in[25], in[26], in[27]);
    const glm::vec3 pt(in[31], in[32], in[33]);
    const glm::vec4 tmp = glm::vec4(pt, 1) * M;
    out[0] = tmp[0] / tmp[3];
    out[1] = tmp[1] / tmp[3];
    out[2] = tmp[2] / tmp[3];
    const glm::mat4 rt(r[0][0], r[0][1], r[0][2], t[0], r[1][0], r[1][1], r[1][2], t[1], r[2][0], r[2][1], r[2][2], t[2], 0.0, 0.0,
                       0.0, 1.0);
    const glm::mat4 inv = glm::inverse(M);
    const glm::mat4 e = inv * rt;
    glm::mat4 K4(0.0);
    K4[0][0] = in[28];
    K4[1][1] = in[28];
    K4[0][2] = in[29];
    K4[1][2] = in[30];
    K4[2][2] = 1.0f;
    const glm::mat4 P = e * K4;
    put(out + 3, inv);
    put(out + 19, e);
    put(out + 35, P);
    fwrite(out, sizeof(float), 51, stdout);
  }
  return 0;
}
