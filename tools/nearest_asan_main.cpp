// nearest_asan_main.cpp — the PLY point reader and the host statement of K18 (include/eg3d/host_nearest.hpp) as a
// stand-alone program for AddressSanitizer + UBSan (tools/asan_nearest_check.sh compiles it with host/ply_read.cpp and
// host/nearest.cpp). It writes well-formed, malformed and truncated PLY files into the directory given as argv[1] — every
// prefix of a binary and of an ASCII file among them —, runs the reader over each, and runs eg3d_host_cloud_nearest on a
// small case whose answers it checks against a brute force. Exit status 0 and "nearest_asan: ok" when everything is as
// expected; the sanitizers end the program themselves on a finding.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "eg3d/host_nearest.hpp"

static int g_bad = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
      g_bad++;                                                    \
    }                                                             \
  } while (0)

static int read_bytes(const std::string& path, const std::string& bytes, uint64_t* n_out, std::vector<float>* pts) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) {
    perror(path.c_str());
    exit(2);
  }
  fwrite(bytes.data(), 1, bytes.size(), f);
  fclose(f);
  float* X = nullptr;
  uint64_t n = 12345;
  const int rc = eg3d_host_read_ply_points(path.c_str(), &X, &n);
  if (rc == 0) {
    if (pts) pts->assign(X, X + 3 * n);
    float sum = 0.f;
    for (uint64_t i = 0; i < 3 * n; i++) sum += X[i];  // (every float the reader promises is touched)
    (void)sum;
    eg3d_host_free_points(X);
    if (n_out) *n_out = n;
  } else {
    EXPECT(X == nullptr && n == 12345);
    EXPECT(strlen(eg3d_host_nearest_last_error()) > 0);
  }
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s SCRATCH_DIRECTORY\n", argv[0]);
    return 2;
  }
  const std::string path = std::string(argv[1]) + "/nearest_asan.ply";
  // ---- the reader
  const std::string head = "ply\nformat ascii 1.0\ncomment c\nelement vertex 3\nproperty uchar r\nproperty float x\nproperty float y\n"
                           "property double w\nproperty float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n";
  const std::string ascii = head + "1 0.5 -1.5 9 2\n2 1e3 4 9 5\r\n3 7 8 9 1e-3\n3 0 1 2\n";
  uint64_t n = 0;
  std::vector<float> pts;
  EXPECT(read_bytes(path, ascii, &n, &pts) == 0 && n == 3 && pts[0] == 0.5f && pts[5] == 5.f && pts[8] == 1e-3f);
  std::string bin = "ply\r\nformat binary_little_endian 1.0\r\nelement vertex 2\r\nproperty uchar r\r\nproperty float x\r\nproperty float y\r\n"
                    "property short s\r\nproperty float z\r\nend_header\r\n";
  const float v[6] = {1.f, 2.f, 3.f, -4.f, 5.5f, 6.f};
  for (int i = 0; i < 2; i++) {
    bin.push_back((char)7);
    bin.append((const char*)&v[3 * i], 8);
    bin.append("\x01\x02", 2);
    bin.append((const char*)&v[3 * i + 2], 4);
  }
  EXPECT(read_bytes(path, bin, &n, &pts) == 0 && n == 2 && pts[3] == -4.f && pts[5] == 6.f);
  // every prefix of both files: refused or read, never a stray access
  int refused = 0;
  for (size_t cut = 0; cut < ascii.size(); cut++) refused += read_bytes(path, ascii.substr(0, cut), nullptr, nullptr) != 0;
  for (size_t cut = 0; cut < bin.size(); cut++) refused += read_bytes(path, bin.substr(0, cut), nullptr, nullptr) != 0;
  EXPECT(refused > 200);
  const char* malformed[] = {
      "", "ply", "ply\n", "plx\nformat ascii 1.0\nend_header\n", "ply\nformat binary_big_endian 1.0\nelement vertex 0\nend_header\n",
      "ply\nformat ascii 2.0\nend_header\n", "ply\nformat ascii 1.0\nend_header\n", "ply\nformat ascii 1.0\nelement vertex\nend_header\n",
      "ply\nformat ascii 1.0\nelement vertex -1\nproperty float x\nproperty float y\nproperty float z\nend_header\n",
      "ply\nformat ascii 1.0\nelement vertex 99999999999999999999999\nproperty float x\nproperty float y\nproperty float z\nend_header\n",
      "ply\nformat ascii 1.0\nelement vertex 18446744073709551615\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 2 3\n",
      "ply\nformat binary_little_endian 1.0\nelement vertex 6148914691236517205\nproperty float x\nproperty float y\nproperty float z\nend_header\nabcdefghijkl",
      "ply\nformat ascii 1.0\nelement vertex 1\nproperty list uchar int x\nend_header\n",
      "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n1 2\n",
      "ply\nformat ascii 1.0\nelement vertex 1\nproperty int x\nproperty float y\nproperty float z\nend_header\n1 2 3\n",
      "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 1 2 3\n",
      "ply\nformat ascii 1.0\nelement vertex 1\nproperty quad x\nend_header\n", "ply\nformat ascii 1.0\nproperty float x\nend_header\n",
      "ply\nformat ascii 1.0\nelement face 1\nproperty int a\nelement vertex 1\nproperty float x\nend_header\n",
      "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 2 z\n",
      "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 2 3abc\n",
      "ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n1 2 3\n4 5 6\n",
  };
  for (const char* m : malformed) EXPECT(read_bytes(path, m, nullptr, nullptr) == EG3D_NEAREST_ERR_PLY);
  {
    std::string nul = "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 2";
    nul.push_back('\0');
    nul += "3 4\n";
    EXPECT(read_bytes(path, nul, nullptr, nullptr) == EG3D_NEAREST_ERR_PLY);
  }
  float* X = nullptr;
  EXPECT(eg3d_host_read_ply_points((std::string(argv[1]) + "/no_such_file.ply").c_str(), &X, &n) == EG3D_NEAREST_ERR_FILE);
  remove(path.c_str());

  // ---- the statement on one small case, against a brute force written here
  std::vector<float> R, Q;
  std::vector<uint8_t> rk, qk;
  uint32_t seed = 12345;
  auto rnd = [&seed]() {
    seed = seed * 1664525u + 1013904223u;
    return (float)(seed >> 8) / 16777216.f;
  };
  for (int i = 0; i < 700; i++) {
    for (int a = 0; a < 3; a++) R.push_back(rnd() * 2.f - 1.f);
    rk.push_back(i % 11 != 0);
  }
  for (int i = 0; i < 900; i++) {
    for (int a = 0; a < 3; a++) Q.push_back(rnd() * 2.4f - 1.2f);
    qk.push_back(i % 13 != 0);
  }
  R[30] = NAN, R[61] = INFINITY, Q[12] = -INFINITY, Q[40] = NAN;
  const float cell = 0.25f, md = 0.2f, md2 = md * md;
  std::vector<float> d2(900);
  std::vector<uint32_t> nn(900);
  eg3d_nearest_stats st;
  memset(&st, 0, sizeof(st));
  st.struct_size = sizeof(st);
  st.n_thresholds = 2;
  st.thresholds[0] = 0.2f, st.thresholds[1] = 0.05f;
  EXPECT(eg3d_host_cloud_nearest(R.data(), 700, rk.data(), Q.data(), 900, qk.data(), cell, md, d2.data(), nn.data(), &st) == 0);
  uint64_t within = 0;
  for (int i = 0; i < 900; i++) {
    float best = INFINITY;
    uint32_t bj = EG3D_NEAREST_NONE;
    const bool ok = qk[i] && std::isfinite(Q[3 * i]) && std::isfinite(Q[3 * i + 1]) && std::isfinite(Q[3 * i + 2]);
    for (int j = 0; ok && j < 700; j++) {
      if (!rk[j] || !std::isfinite(R[3 * j]) || !std::isfinite(R[3 * j + 1]) || !std::isfinite(R[3 * j + 2])) continue;
      const float dx = Q[3 * i] - R[3 * j], dy = Q[3 * i + 1] - R[3 * j + 1], dz = Q[3 * i + 2] - R[3 * j + 2];
      const float d = (dx * dx + dy * dy) + dz * dz;
      if (d < md2 && d < best) best = d, bj = (uint32_t)j;
    }
    within += bj != EG3D_NEAREST_NONE;
    EXPECT(nn[i] == bj && (d2[i] == best || (std::isinf(d2[i]) && std::isinf(best))));
  }
  EXPECT(st.n_within == within && within > 100 && st.n_queries == 900 && st.n_below[0] == within && st.n_below[1] < within);
  // the refusals write nothing
  eg3d_nearest_stats before = st;
  EXPECT(eg3d_host_cloud_nearest(R.data(), 700, nullptr, Q.data(), 900, nullptr, 0.1f, md, d2.data(), nn.data(), &st) == EG3D_NEAREST_ERR_MAXDIST);
  EXPECT(memcmp(&before, &st, sizeof(st)) == 0);
  eg3d_cloud_index_stats is;
  memset(&is, 0, sizeof(is));
  is.struct_size = sizeof(is);
  EXPECT(eg3d_host_cloud_index_stats(R.data(), 700, rk.data(), cell, &is) == 0 && is.n_nonfinite == 2 && is.n_indexed + is.n_dropped + 2 == 700);
  EXPECT(eg3d_host_cloud_nearest(nullptr, 0, nullptr, Q.data(), 900, nullptr, cell, md, d2.data(), nullptr, nullptr) == 0 && std::isinf(d2[5]));
  if (g_bad) {
    fprintf(stderr, "nearest_asan: %d expectation(s) failed\n", g_bad);
    return 1;
  }
  printf("nearest_asan: ok (%d truncated or malformed files refused, %llu of 900 queries within reach)\n", refused + (int)(sizeof(malformed) / sizeof(malformed[0])) + 1,
         (unsigned long long)within);
  return 0;
}
