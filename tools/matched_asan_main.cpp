// Stand-alone sanitizer run of eg3d_host_is_matched (tools/asan_matched_check.sh builds this file and the host sources it
// needs with -fsanitize=address,undefined and runs it; nothing of it is ever loaded into Python).
//   1. hand-made rows on a 5-vertex polyline, one per rule and quirk of csrc/eg3d_matched_core.h, expected answers asserted;
//      tables that must be refused (and are, before anything is indexed with them);
//   2. the intervals and points of a text file (argv[1]) on synthetic config 0:
//        NP  n_intervals  n_points
//        NP + 1 offsets; per interval "start_seg sx sy end_seg ex ey" (coordinates as float bit patterns, hex);
//        per point "view polyline segment x y expected_index"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "eg3d_host.h"

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);        \
      failures++;                                                 \
    }                                                             \
  } while (0)

struct Iv {
  uint32_t s;
  float sx, sy;
  uint32_t e;
  float ex, ey;
};

struct Table {
  std::vector<uint64_t> off;
  std::vector<uint32_t> sseg, eseg;
  std::vector<float> sxy, exy;
  eg3d_matched_intervals m;
  Table(uint32_t n_pl, uint32_t g, const std::vector<Iv>& row) {
    for (uint32_t i = 0; i <= n_pl; i++) off.push_back(i > g ? row.size() : 0);
    for (const Iv& v : row) {
      sseg.push_back(v.s), eseg.push_back(v.e);
      sxy.push_back(v.sx), sxy.push_back(v.sy), exy.push_back(v.ex), exy.push_back(v.ey);
    }
    std::memset(&m, 0, sizeof(m));
    m.struct_size = sizeof(m);
    m.n_scene_polylines = n_pl;
    m.iv_off = off.data();
    m.iv_start_seg = sseg.data();
    m.iv_start_xy = sxy.data();
    m.iv_end_seg = eseg.data();
    m.iv_end_xy = exy.data();
  }
};

static int64_t ask(const eg3d_scene& sc, const std::vector<Iv>& row, uint32_t seg, float x, float y, int* rc_out = nullptr) {
  Table t(sc.view_pl_off[1], 0, row);
  const int32_t view = 0;
  const uint32_t pl = 0;
  const float xy[2] = {x, y};
  int64_t k = -99;
  const int rc = eg3d_host_is_matched(&sc, &t.m, 1, &view, &pl, &seg, xy, &k);
  if (rc_out) *rc_out = rc;
  return rc == -1 ? -99 : k;
}

static void hand_made() {
  const float vtx[] = {0, 0, 100, 0, 200, 0, 300, 0, 400, 0, 7, 7};
  const uint32_t vpo[] = {0, 2}, pvo[] = {0, 5, 6}, ps[] = {0, 2}, pe[] = {1, 2};
  const uint8_t valid[] = {1, 1};
  eg3d_scene sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.n_views = 1;
  sc.view_pl_off = vpo;
  sc.pl_vtx_off = pvo;
  sc.vtx_xy = vtx;
  sc.pl_start = ps;
  sc.pl_end = pe;
  sc.pl_valid = valid;
  const Iv A1{1, 110, 0, 1, 150, 0}, B2{2, 220, 0, 2, 260, 0}, Z0{0, 10, 0, 0, 50, 0}, LONG{1, 110, 0, 3, 350, 0},
      A12{1, 110, 0, 2, 250, 0}, ENDV{1, 110, 0, 1, 200, 0}, STARTV{2, 200, 0, 2, 260, 0}, BACK{2, 210, 0, 1, 120, 0};
  CHECK(ask(sc, {Z0}, 0, 30, 0) == -1);          // M1
  CHECK(ask(sc, {LONG}, 2, 250, 0) == -1);       // M2
  CHECK(ask(sc, {A1, B2}, 2, 240, 0) == 1);      // M3: own segment
  CHECK(ask(sc, {A1, B2}, 2, 210, 0) == -1);
  CHECK(ask(sc, {A12}, 2, 230, 0) == 0);         // M3: the one before
  CHECK(ask(sc, {A12}, 2, 270, 0) == -1);
  CHECK(ask(sc, {B2}, 1, 150, 0) == -1);         // M4
  CHECK(ask(sc, {A1}, 1, 130, 0) == 0);
  CHECK(ask(sc, {A1}, 1, 105, 0) == -1);
  CHECK(ask(sc, {A1}, 1, 160, 0) == -1);
  CHECK(ask(sc, {ENDV}, 2, 200, 0) == 0);        // on the end vertex, tagged with the next segment
  CHECK(ask(sc, {STARTV}, 1, 200, 0) == -1);     // on the start vertex, tagged with the previous segment
  CHECK(ask(sc, {Z0, STARTV}, 1, 200, 0) == -1);
  CHECK(ask(sc, {}, 1, 130, 0) == -1);
  int rc = 0;
  CHECK(ask(sc, {BACK}, 2, 250, 0, &rc) == -2 && rc == -2);  // the walk would not advance: index 0 as -2 - 0
  // refused tables and points
  CHECK(ask(sc, {B2, A1}, 1, 130, 0) == -99);
  CHECK(ask(sc, {A1, Iv{1, 160, 0, 1, 170, 0}}, 1, 130, 0) == -99);
  CHECK(ask(sc, {Iv{4, 400, 0, 4, 400, 0}}, 1, 130, 0) == -99);
  CHECK(ask(sc, {Iv{1, 110, 0, 4, 400, 0}}, 1, 130, 0) == -99);
  CHECK(ask(sc, {A1}, 4, 400, 0) == -99);
  {
    Table t(2, 1, {Iv{0, 7, 7, 0, 7, 7}});  // an interval on the one-vertex polyline
    const int32_t view = 0;
    const uint32_t pl = 0, seg = 1;
    const float xy[2] = {130, 0};
    int64_t k;
    CHECK(eg3d_host_is_matched(&sc, &t.m, 1, &view, &pl, &seg, xy, &k) == -1);
    Table u(2, 0, {A1});
    u.off[1] = 5;  // an offset past the total
    CHECK(eg3d_host_is_matched(&sc, &u.m, 1, &view, &pl, &seg, xy, &k) == -1);
    u.off[1] = 1;
    u.m.struct_size = 8;
    CHECK(eg3d_host_is_matched(&sc, &u.m, 1, &view, &pl, &seg, xy, &k) == -1);
  }
}

static float from_bits(unsigned u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

static void from_file(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    failures++;
    return;
  }
  unsigned long long np = 0, ni = 0, npts = 0;
  CHECK(std::fscanf(f, "%llu %llu %llu", &np, &ni, &npts) == 3);
  std::vector<uint64_t> off(np + 1);
  for (auto& o : off) {
    unsigned long long v = 0;
    CHECK(std::fscanf(f, "%llu", &v) == 1);
    o = v;
  }
  std::vector<uint32_t> sseg(ni + 1), eseg(ni + 1);
  std::vector<float> sxy(2 * ni + 2), exy(2 * ni + 2);
  for (unsigned long long i = 0; i < ni; i++) {
    unsigned a, b, c, d, e2, g;
    CHECK(std::fscanf(f, "%u %x %x %u %x %x", &a, &b, &c, &d, &e2, &g) == 6);
    sseg[i] = a, eseg[i] = d;
    sxy[2 * i] = from_bits(b), sxy[2 * i + 1] = from_bits(c), exy[2 * i] = from_bits(e2), exy[2 * i + 1] = from_bits(g);
  }
  std::vector<int32_t> view(npts + 1);
  std::vector<uint32_t> pl(npts + 1), seg(npts + 1);
  std::vector<float> xy(2 * npts + 2);
  std::vector<int64_t> want(npts + 1), got(npts + 1, -77);
  for (unsigned long long i = 0; i < npts; i++) {
    int v;
    unsigned p, s, x, y;
    long long w;
    CHECK(std::fscanf(f, "%d %u %u %x %x %lld", &v, &p, &s, &x, &y, &w) == 6);
    view[i] = v, pl[i] = p, seg[i] = s, xy[2 * i] = from_bits(x), xy[2 * i + 1] = from_bits(y), want[i] = w;
  }
  std::fclose(f);
  eg3d_synth_config cfg;
  eg3d_synth_default_config(&cfg, 0);
  eg3d_synth* syn = eg3d_synth_create(&cfg);
  const eg3d_scene* sc = eg3d_synth_scene(syn);
  CHECK(sc->view_pl_off[sc->n_views] == np);
  eg3d_matched_intervals m;
  std::memset(&m, 0, sizeof(m));
  m.struct_size = sizeof(m);
  m.n_scene_polylines = np;
  m.iv_off = off.data();
  m.iv_start_seg = sseg.data();
  m.iv_start_xy = sxy.data();
  m.iv_end_seg = eseg.data();
  m.iv_end_xy = exy.data();
  CHECK(eg3d_host_is_matched(sc, &m, npts, view.data(), pl.data(), seg.data(), xy.data(), got.data()) == 0);
  unsigned long long matched = 0;
  for (unsigned long long i = 0; i < npts; i++) {
    CHECK(got[i] == want[i]);
    matched += got[i] >= 0;
  }
  std::printf("synthetic config 0: %llu intervals, %llu points, %llu inside a held interval\n", ni, npts, matched);
  CHECK(matched > 0);
  eg3d_synth_destroy(syn);
}

int main(int argc, char** argv) {
  hand_made();
  if (argc > 1) from_file(argv[1]);
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
