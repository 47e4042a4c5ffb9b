/*
 * eg3d_probe.h — TEST-ONLY entry points of tests/probe/libeg3d_probe.so: single device primitives of
 * the product's headers run on the GPU, for the bit-for-bit arithmetic checks of
 * tests/test_gpu_arith.py, the lane-group solver checks of tests/test_gpu_coop_gn.py, the glm pin of tests/test_glm_pin.py
 * and the item-by-item checks of the geometry and walk primitives of tests/test_gpu_geom_primitives.py (the walks in all
 * their forms, the segment / line tests, the grid-cell rounding, the closest-point scans, the epipolar line; tables from
 * tests/geom_cases.py, reference rows from the oracle, tests/test_geom_cases.py). Not part of the product and not linked
 * into libeg3d.so.
 */
#ifndef EG3D_PROBE_H_
#define EG3D_PROBE_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* out_d[5][n]: a/b, sqrt(|a|), a*b+c (two roundings), (double)(float)a, 1/sqrt; out_f likewise in float */
int eg3d_probe_arith(uint64_t n, const double* a, const double* b, const double* c, double* out_d, const float* fa,
                     const float* fb, const float* fc, float* out_f);
/* n_cases triangulations of k observations each; cam_P = [n_views][16] host array */
int eg3d_probe_dlt_rows(void); /* the DLT form the probe was compiled with (EG3D_DLT_ROWS) */
int eg3d_probe_triangulate(const float* cam_P, int n_views, uint64_t n_cases, int k, const int32_t* views, const float* xy,
                           float* X, uint8_t* valid, double* dlt_X0);
/* the same 2-view DLTs (minimum view id, last observation) on groups of 8 lanes (dlt2_grp8, eg3d_dev_coopgn.h) */
int eg3d_probe_dlt_groups(const float* cam_P, int n_views, uint64_t n_cases, int k, const int32_t* views, const float* xy,
                          double* dlt_X0);
/* the shared-reciprocal division of the Gauss-Newton rows: out[0..n) = num/den, out[n..2n) = gn_div(num, gn_recip(den)),
 * out[2n..3n) = 1.0 where den is in the admitted range */
int eg3d_probe_gn_div(uint64_t n, const double* num, const double* den, double* out3n);
/* GnRow (j00 j01 j02 j10 j11 j12 r0 r1) of n rows with the plain divisions (out[0..8n)) and through the guarded fast
 * path (out[8n..16n)); P16 = one 4x4 camera matrix per row */
int eg3d_probe_gn_rows(uint64_t n, const float* P16, const float* oxy, const double* X, double* out16n);
/* the lane-group Gauss-Newton solver at full density (tools/gn_floor.py): n_blocks single-wave blocks x rounds windows of
 * seven identical ADD requests of n <= 9 rows; *ms = kernel time; X_ok = {mean solution x of block 0, its accepted solves} */
int eg3d_probe_gn_dense(const float* cam_P, int n_views, const int32_t* obs_view, const float* obs_xy, int n,
                        const float* X0, int n_blocks, int rounds, float* ms, float* X_ok);
/* the lane-group Gauss-Newton solver (coop_gn_groups, eg3d_dev_coopgn.h) on windows of up to 32 requests, one single-wave
 * block per window, as the expand kernel calls it (tests/test_gpu_coop_gn.py). variant: 0 small <0, false, 30>, 1 general
 * <0, true, 30>, 2 many views <EG3D_MANY_KEEP, true, EG3D_GN_PRECHECK_IT> (the product's three instantiations), 3 <2, true,
 * EG3D_GN_PRECHECK_IT> (KEEP = 2), 4 <0, true, EG3D_GN_PRECHECK_IT> and 5 <0, false, EG3D_GN_PRECHECK_IT>
 * (EG3D_GN_PRECHECK_ALL). Request j of window w = entry w * 32 + j: req_i = {want, offset, nblock, has_extra, extra view},
 * req_f = {extra x, extra y, X0[3]}; rows offset .. offset + nblock - 1 of obs_view / obs_xy, then the extra one.
 * Out per entry: valid, X[3] and the group size G its request was solved with (0 = not solved: not wanted, or a long
 * request refused), per window long_refused. Returns 0, -1 on bad arguments, -2 on a HIP error. */
int eg3d_probe_coop_gn(int variant, const float* cam_P, int n_views, const int32_t* obs_view, const float* obs_xy,
                       uint64_t n_obs, int n_windows, const int32_t* req_i, const float* req_f, int cams_mid_range,
                       uint8_t* valid, float* X, int32_t* G, uint8_t* long_refused);
int eg3d_probe_coop_gn_variants(void); /* number of variants */
/* 2-D geometry primitives on the GPU (tests/test_glm_pin.py): mode 0 project_f32 (in [n][19] = P16 + X -> [n][2]),
 * 1 seg_line_cos (in [n][7] = segment + line -> [n]), 2 seg_closest (in [n][6] = p, v, w -> [n][3] = d2, closest point) */
int eg3d_probe_geom(uint64_t n, int mode, const float* in, float* out);

/* ---- the geometry and walk primitives of eg3d_dev_geom.h and epiline (eg3d_dev_tri.h), item by item
 * (tests/test_gpu_geom_primitives.py): one row per lane, one primitive call per row, through the items of eg3d_geom_items.h
 * that tests/hostsim runs through the HOST compilation of the same headers (hostsim_geom_*: same arguments). The outputs are
 * read and written in place: the caller fills them with a sentinel, and what a primitive leaves untouched comes back as the
 * sentinel. All return 0, -1 when a table breaks the input contract (nothing is launched then: a polyline of fewer than 2
 * vertices, offsets not ascending or outside the vertex array, seg > n - 2, s0 / s1 > n - 1, a vertex or segment row that is
 * not finite, the wrong number of boxes), the positive code of hipGetLastError() when the launch itself fails, -2 on any other
 * HIP error.
 * Polylines: vtx = [nv + 1][2], ONE SPARE VERTEX behind the nv used ones; polyline p = vertices pl_off[p] .. pl_off[p + 1] - 1.
 *
 * eg3d_probe_walk: one walk step per row. form 0 walk_by_distance, 1 walk_by_distance_pf, 2 walk_by_line (global pointer),
 * 3 walk_by_line on PlRefT<const address_space(3) f2*> (one polyline per block, staged in LDS first; rows must be grouped by
 * polyline, ascending, and no polyline may exceed eg3d_probe_walk_lds_capacity() vertices), 4 walk_by_line_pf, 5..8
 * walk_by_line_head<1..4> followed in the same lane by walk_seg_test over k < left and walk_resolve. row_f = [n][8]: x, y of the
 * start point, la, lb, lc, distance, min_d, max_d; row_dir = the node id walked towards; row_bnd = bounded walk. */
int eg3d_probe_walk(int form, const float* vtx, uint64_t nv, const uint32_t* pl_off, const uint32_t* pl_start,
                    const uint32_t* pl_end, uint32_t npl, uint64_t n, const uint32_t* row_pl, const uint32_t* row_seg,
                    const uint32_t* row_dir, const float* row_f, const uint8_t* row_bnd, uint32_t* status, uint32_t* seg,
                    float* xy);
int eg3d_probe_walk_lds_capacity(void);
/* in = [n][8]: x1 y1 x2 y2 la lb lc thr. mode 0 seg_line_hit (r = found, o = the hit), 1 seg_line_hit_guarded (r = its bits,
 * o = the hit), 2 point_line_dist of (x1, y1) (o[0]), 3 r = bit 0 seg_line_cos_gt(..., thr), bit 1 seg_line_cos(...) > thr
 * evaluated in the same kernel, o[0] = seg_line_cos */
int eg3d_probe_seg(int mode, uint64_t n, const float* in, uint32_t* r, float* o2);
/* in = [n][3]: cell x y; dims = [n][4]: img_w img_h map_w map_h (mode 1). mode 0 cell_of -> col row bx by, 1 cell_window ->
 * c0 c1 r0 r1 */
int eg3d_probe_cells(int mode, uint64_t n, const float* in, const int32_t* dims, int32_t* out4);
/* mode 0 polyline_closest, 1 polyline_closest_range [s0, s1), 2 polyline_closest_pruned with the boxes bb = [nbb][4] (blocks
 * of EG3D_BB_SEGS segments; polyline p's boxes start at bb_off[p]). q = [n][2] query points (NaN / infinite allowed). */
int eg3d_probe_closest(int mode, const float* vtx, uint64_t nv, const uint32_t* pl_off, uint32_t npl, const float* bb,
                       uint64_t nbb, const uint32_t* bb_off, uint64_t n, const uint32_t* row_pl, const uint32_t* row_s0,
                       const uint32_t* row_s1, const float* q, float* d, uint32_t* seg, float* xy);
/* epiline with one matrix F = [n][9] and one validity byte per row */
int eg3d_probe_epiline(uint64_t n, const double* F, const uint8_t* valid, const float* xy, int32_t* ok, float* line3);
#ifdef __cplusplus
}
#endif
#endif
