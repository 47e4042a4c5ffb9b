// TEST-ONLY: the cooperative form of walk_by_line (eg3d_dev_geom.h: head, per-segment body, resolve) run on the
// host the way a wavefront runs it, behind a tiny C interface (tests/test_walk_coop.py compares it with walk_by_line).
// The 64 lanes of a pass are a loop over k: every lane's test is evaluated (as on the device, where all lanes run
// before the ballot), and the first decisive k in walking order decides.
#include "eg3d_dev_geom.h"

using namespace eg3d;

namespace {
template <int T>
uint32_t coop(const PlRef& pl, const PlPt& p, uint32_t dir, float la, float lb, float lc, bool bounded, float min_d,
              float max_d, PlPt& out, uint32_t* passes) {
  const LineDir ld = line_dir(la, lb);
  WalkCont c;
  c.next = c.left = 0;
  c.step = 1;
  uint32_t status = walk_by_line_head<T>(pl, p, dir, la, lb, lc, ld, bounded, min_d, max_d, out, c);
  if (status != WALK_UNDECIDED) return status;
  uint32_t rf = 0, sf = 0;
  float xf = 0.0f, yf = 0.0f;
  for (int32_t k0 = 0; k0 < c.left && !rf; k0 += 64) {
    ++*passes;
    uint32_t r[64], seg[64];
    float hx[64], hy[64];
    for (int32_t lane = 0; lane < 64; lane++) {
      r[lane] = seg[lane] = 0;
      hx[lane] = hy[lane] = 0.0f;
      const int32_t k = k0 + lane;
      if (k < c.left) r[lane] = walk_seg_test(pl.v, c, k, la, lb, lc, ld, seg[lane], hx[lane], hy[lane]);
    }
    for (int32_t lane = 0; lane < 64; lane++)
      if (r[lane]) {
        rf = r[lane];
        sf = seg[lane];
        xf = hx[lane];
        yf = hy[lane];
        break;
      }
  }
  return walk_resolve(rf, sf, xf, yf, p, bounded, min_d, max_d, out);
}
}  // namespace

// out4 = {status, seg, bits of x, bits of y} (seg / x / y keep the caller's sentinel where the walk does not write them)
extern "C" void walkcoop_ref(const float* vtx, uint32_t n, uint32_t start, uint32_t end, uint32_t seg, float x, float y,
                             uint32_t dir, float la, float lb, float lc, int bounded, float min_d, float max_d,
                             uint32_t* out4) {
  PlRef pl;
  pl.v = (const f2*)vtx;
  pl.n = n;
  pl.start = start;
  pl.end = end;
  PlPt p{seg, x, y}, o;
  o.seg = out4[1];
  __builtin_memcpy(&o.x, &out4[2], 4);
  __builtin_memcpy(&o.y, &out4[3], 4);
  out4[0] = walk_by_line(pl, p, dir, la, lb, lc, bounded != 0, min_d, max_d, o);
  out4[1] = o.seg;
  __builtin_memcpy(&out4[2], &o.x, 4);
  __builtin_memcpy(&out4[3], &o.y, 4);
}

// the same through head (T whole segments) + passes of 64 + resolve; *passes counts the passes made
extern "C" int walkcoop_run(int T, const float* vtx, uint32_t n, uint32_t start, uint32_t end, uint32_t seg, float x, float y,
                            uint32_t dir, float la, float lb, float lc, int bounded, float min_d, float max_d, uint32_t* out4,
                            uint32_t* passes) {
  PlRef pl;
  pl.v = (const f2*)vtx;
  pl.n = n;
  pl.start = start;
  pl.end = end;
  PlPt p{seg, x, y}, o;
  o.seg = out4[1];
  __builtin_memcpy(&o.x, &out4[2], 4);
  __builtin_memcpy(&o.y, &out4[3], 4);
  *passes = 0;
  const bool b = bounded != 0;
  switch (T) {
    case 1: out4[0] = coop<1>(pl, p, dir, la, lb, lc, b, min_d, max_d, o, passes); break;
    case 2: out4[0] = coop<2>(pl, p, dir, la, lb, lc, b, min_d, max_d, o, passes); break;
    case 3: out4[0] = coop<3>(pl, p, dir, la, lb, lc, b, min_d, max_d, o, passes); break;
    case 4: out4[0] = coop<4>(pl, p, dir, la, lb, lc, b, min_d, max_d, o, passes); break;
    default: return -1;
  }
  out4[1] = o.seg;
  __builtin_memcpy(&out4[2], &o.x, 4);
  __builtin_memcpy(&out4[3], &o.y, 4);
  return 0;
}

// Batch form (the Python loop over every start segment is the slow part): for every start segment s of the polyline, both
// directions and a direction that is neither end, bounded and unbounded, the position at fraction `frac` of the segment:
// compare and count mismatches; *n_cases, *n_long (walks that left the head), *n_multi (walks of more than one pass).
extern "C" int walkcoop_sweep(int T, const float* vtx, uint32_t n, float frac, float la, float lb, float lc, float min_d,
                              float max_d, uint32_t* n_cases, uint32_t* n_long, uint32_t* n_multi) {
  int bad = 0;
  const uint32_t start = 7, end = 9, neither = 8;
  const uint32_t dirs[3] = {start, end, neither};
  for (uint32_t s = 0; s + 1 < n; s++) {
    const float x = vtx[2 * s] + frac * (vtx[2 * s + 2] - vtx[2 * s]);
    const float y = vtx[2 * s + 1] + frac * (vtx[2 * s + 3] - vtx[2 * s + 1]);
    for (int d = 0; d < 3; d++)
      for (int b = 0; b < 2; b++) {
        uint32_t a4[4] = {0, 0xdeadbeefu, 0x7fc12345u, 0x7fc54321u}, b4[4] = {0, 0xdeadbeefu, 0x7fc12345u, 0x7fc54321u};
        uint32_t passes = 0;
        walkcoop_ref(vtx, n, start, end, s, x, y, dirs[d], la, lb, lc, b, min_d, max_d, a4);
        if (walkcoop_run(T, vtx, n, start, end, s, x, y, dirs[d], la, lb, lc, b, min_d, max_d, b4, &passes)) return -1;
        ++*n_cases;
        if (passes >= 1) ++*n_long;
        if (passes >= 2) ++*n_multi;
        if (a4[0] != b4[0] || a4[1] != b4[1] || a4[2] != b4[2] || a4[3] != b4[3]) bad++;
      }
  }
  return bad;
}
