// eg3d_host_is_matched: the host instantiation of csrc/eg3d_matched_core.h behind a batched C probe — what the kernels
// of eg3d_match_polyline_sets_matched evaluate per sample and per epipolar hit, callable without a GPU.
#include <stdint.h>

#include "eg3d_host.h"
#include "eg3d_matched_core.h"

using namespace eg3d;

namespace {

IvTable table_of(const eg3d_matched_intervals* m) {
  IvTable t;
  t.off = m->iv_off;
  t.start_seg = m->iv_start_seg;
  t.start_xy = m->iv_start_xy;
  t.end_seg = m->iv_end_seg;
  t.end_xy = m->iv_end_xy;
  return t;
}

}  // namespace

// the host statement of the table check the device runs (k_n1_check_intervals), one loop instead of one lane per row
// (the vertices an invalid polyline may still carry in the input are ignored, as everywhere: include/eg3d.h pl_valid)
static uint32_t n_vtx_of(const uint32_t* pl_vtx_off, const uint8_t* pl_valid, uint32_t g) {
  return pl_valid && !pl_valid[g] ? 0u : pl_vtx_off[g + 1] - pl_vtx_off[g];
}
extern "C" int eg3d_host_check_matched_intervals(const uint32_t* view_pl_off, int32_t n_views, const uint32_t* pl_vtx_off,
                                                 const uint8_t* pl_valid, const eg3d_matched_intervals* m) {
  if (!m || !view_pl_off || !pl_vtx_off || n_views < 1) return -1;
  if (m->struct_size != sizeof(eg3d_matched_intervals) || m->on_device) return -1;
  const uint32_t NP = view_pl_off[n_views];
  if (m->n_scene_polylines != NP || !m->iv_off) return -1;
  const uint64_t total = m->iv_off[NP];
  if (total && (!m->iv_start_seg || !m->iv_start_xy || !m->iv_end_seg || !m->iv_end_xy)) return -1;
  const IvTable t = table_of(m);
  for (uint32_t g = 0; g < NP; g++)
    if (!check_interval_row(t, total, g, n_vtx_of(pl_vtx_off, pl_valid, g))) return -1;
  return 0;
}

extern "C" int eg3d_host_is_matched(const eg3d_scene* sc, const eg3d_matched_intervals* m, uint64_t n, const int32_t* view,
                                    const uint32_t* pl, const uint32_t* seg, const float* xy, int64_t* out_index) {
  if (!sc || !m || sc->n_views < 1 || !sc->view_pl_off || !sc->pl_vtx_off || !sc->vtx_xy || !sc->pl_start || !sc->pl_end)
    return -1;
  if (n && (!view || !pl || !seg || !xy || !out_index)) return -1;
  if (eg3d_host_check_matched_intervals(sc->view_pl_off, sc->n_views, sc->pl_vtx_off, sc->pl_valid, m) != 0) return -1;
  for (uint64_t i = 0; i < n; i++) {
    if (view[i] < 0 || view[i] >= sc->n_views) return -1;
    if (pl[i] >= sc->view_pl_off[view[i] + 1] - sc->view_pl_off[view[i]]) return -1;
    const uint32_t g = sc->view_pl_off[view[i]] + pl[i];
    const uint32_t nv = n_vtx_of(sc->pl_vtx_off, sc->pl_valid, g);
    if (nv < 2 || seg[i] >= nv - 1) return -1;
  }
  const IvTable t = table_of(m);
  int rc = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t g = sc->view_pl_off[view[i]] + pl[i];
    PlRef ref;
    ref.v = reinterpret_cast<const f2*>(sc->vtx_xy) + sc->pl_vtx_off[g];
    ref.n = sc->pl_vtx_off[g + 1] - sc->pl_vtx_off[g];
    ref.start = sc->pl_start[g];
    ref.end = sc->pl_end[g];
    PlPt p;
    p.seg = seg[i];
    p.x = xy[2 * i];
    p.y = xy[2 * i + 1];
    const IvRow row = iv_row(t, g);
    const int32_t k = is_matched(row, ref.v, p);
    out_index[i] = k;
    if (k < 0) continue;
    // the extractor goes on from next_pl_point_by_distance(interval.end, pl.end, 20): it must get past p. (A closed
    // polyline, start node == end node, yields no sample — the walk tests `direction == start` first and stops at
    // once — so nothing ever jumps on it: only its hits are asked about.)
    if (ref.start == ref.end) continue;
    PlPt e, q;
    e.seg = row.end_seg[k];
    e.x = row.end_xy[2 * k];
    e.y = row.end_xy[2 * k + 1];
    const uint32_t w = walk_by_distance(ref, e, ref.end, 20.0f, q);
    if (!(w & WALK_EXTREME) && !walk_progresses(ref.v, p, q)) {
      out_index[i] = -2 - (int64_t)k;
      rc = -2;
    }
  }
  return rc;
}
