"""CPU half of the item-by-item check of the geometry and walk primitives (edgegraph3d_amd/csrc/eg3d_dev_geom.h, epiline of
eg3d_dev_tri.h): the tables of tests/geom_cases.py, their reference rows from the oracle alone (tests/geom_ref.py), and
(1) the HOST compilation of the header (tests/hostsim: hostsim_geom_*) equals those rows bit for bit — status, segment, the
bits of every coordinate, what is left untouched included; (2) the coverage conditions hold on the reference rows, so that
they are settled before any GPU runs. tests/test_gpu_geom_primitives.py then holds the gfx950 compilation to the same rows:
when this file passes, a failure there is the device build's."""
import numpy as np
import pytest

import geom_cases as gc
import geom_ref as gr


@pytest.fixture(scope="module")
def hs():
    import hostsim_binding
    return gr.bind(hostsim_binding.lib(), "hostsim_geom_")


def test_tables_respect_the_input_contract():
    w, c = gc.walk_table(), gc.closest_table()
    for t in (w, c):
        assert np.isfinite(t.vtx).all() and np.abs(t.vtx).max() <= 1e7 and (np.diff(t.pl_off.astype(np.int64)) >= 2).all()
        assert t.pl_off[-1] == t.nv == len(t.vtx) - 1          # one spare vertex behind the last polyline
    assert sorted(set(w.pl_size.tolist())) == sorted(gc.SIZES) and set(w.pl_shape) == set(gc.SHAPES)
    assert w.pl_loop.any() and (~w.pl_loop).any() and w.pl_scaled.any()
    assert np.abs(w.vtx[w.pl_off[np.flatnonzero(w.pl_scaled)[0]]:]).max() > 5e5
    assert (w.row_seg <= w.row_size - 2).all()
    # the start points lie on their segments (within the rounding of the interpolation)
    a, b = w.vtx[w.pl_off[w.row_pl] + w.row_seg].astype(np.float64), w.vtx[w.pl_off[w.row_pl] + w.row_seg + 1].astype(np.float64)
    p = w.row_f[:, 0:2].astype(np.float64)
    d = np.abs(np.hypot(*(p - a).T) + np.hypot(*(b - p).T) - np.hypot(*(b - a).T))
    assert (d <= 1e-5 * np.maximum(1.0, np.abs(p).max(1))).all()
    for k in (gc.DIR_START, gc.DIR_END, gc.DIR_NEITHER):
        assert (w.row_dirkind == k).sum() > 1000
    assert set(np.unique(w.row_f[:, 5]).tolist()) == set(np.float32(gc.DISTANCES).tolist())
    assert 10000 <= w.n <= 60000 and (w.row_f[:, 3] == 0).sum() >= 100       # lines with lb == 0
    first, last = w.row_seg == 0, w.row_seg == w.row_size - 2
    assert first.sum() > 1000 and last.sum() > 1000 and (~first & ~last).sum() > 1000
    on_vertex = (w.row_f[:, 0:2] == w.vtx[w.pl_off[w.row_pl] + w.row_seg]).all(1)
    at_one = (w.row_f[:, 0:2] == w.vtx[w.pl_off[w.row_pl] + w.row_seg + 1]).all(1)
    assert on_vertex.sum() > 1000 and at_one.sum() > 1000
    assert (c.row_s1 <= (c.pl_off[1:] - c.pl_off[:-1] - 1)[c.row_pl]).all() and set(c.pl_kind) == set(gc.CLOSEST_KINDS)
    assert (~np.isfinite(c.q)).any(1).sum() >= 100
    s = gc.seg_table()
    assert ((s.rows[:, 0] == s.rows[:, 2]) & (s.rows[:, 1] == s.rows[:, 3])).sum() >= 600      # zero-length segments
    den0 = (s.rows[:, 4] * (s.rows[:, 2] - s.rows[:, 0]) + s.rows[:, 5] * (s.rows[:, 3] - s.rows[:, 1])) == 0
    nonzero = (s.rows[:, 0] != s.rows[:, 2]) | (s.rows[:, 1] != s.rows[:, 3])
    assert (den0 & nonzero).sum() >= 50                      # den == 0 exactly: axis-aligned segment, axis-aligned line


def test_coverage_of_the_walk_tables():
    ref = gr.reference()
    gr.walk_coverage(ref.walk_dist, ref.walk_line)


def test_coverage_of_the_segment_cell_closest_and_epiline_tables():
    ref = gr.reference()
    gr.seg_coverage(ref.seg)
    gr.cell_coverage(ref.cells)
    gr.window_coverage(ref.cells)
    gr.closest_coverage(ref.closest)
    gr.closest_coverage(ref.closest, gr.whole_range_rows(), ranges=False)
    gr.epiline_coverage(ref.epiline)


@pytest.mark.parametrize("form", [f for f in gr.WALK_FORMS if f != gr.LDS_FORM], ids=lambda f: gr.WALK_FORMS[f])
def test_host_walks_equal_the_oracle(hs, form):
    """(the address_space(3) instantiation does not exist on the host: tests/test_gpu_geom_primitives.py)"""
    ref = gr.reference()
    r = ref.walk_dist if form in gr.DISTANCE_FORMS else ref.walk_line
    got = gr.run_walk(hs, form)
    gr.assert_rows_equal(gr.WALK_FORMS[form], {"status": r.status, "seg": r.seg, "xy": r.xy},
                         {"status": got.status, "seg": got.seg, "xy": got.xy}, gr.walk_inputs())


def test_host_segment_tests_equal_the_oracle(hs):
    ref, t = gr.reference().seg, gc.seg_table()
    inp = {"row": t.rows}
    got = gr.run_seg(hs, gr.SEG_HIT, t.rows)
    gr.assert_rows_equal("seg_line_hit", {"r": ref.hit.r, "hit": ref.hit.o}, {"r": got.r, "hit": got.o}, inp)
    got = gr.run_seg(hs, gr.SEG_GUARDED, t.rows)
    gr.assert_rows_equal("seg_line_hit_guarded", {"r": ref.guarded.r, "hit": ref.guarded.o}, {"r": got.r, "hit": got.o}, inp)
    got = gr.run_seg(hs, gr.SEG_PLDIST, t.points)
    gr.assert_rows_equal("point_line_dist", {"d": ref.pldist}, {"d": got.o[:, 0].copy()}, {"row": t.points})
    got = gr.run_seg(hs, gr.SEG_COS_GT, t.rows)
    gr.check_cos_gt(ref, got, t)


def test_host_cells_equal_the_oracle(hs):
    """cell_of's (col, row, bx, by) = orc_cell_from_coords' (col, row, on_boundary_row, on_boundary_col): the reference names
    the flag of x "row" and the flag of y "col" (polymatch_ref.cell_from_coords)"""
    ref, t = gr.reference().cells, gc.cell_table()
    gr.assert_rows_equal("cell_of", {"cell": ref.of}, {"cell": gr.run_cells(hs, gr.CELL_OF)}, {"row": t.rows})
    gr.assert_rows_equal("cell_window", {"window": ref.window}, {"window": gr.run_cells(hs, gr.CELL_WINDOW)},
                         {"row": t.wrows, "dims": t.wdims})


@pytest.mark.parametrize("mode", [gr.CLOSEST_WHOLE, gr.CLOSEST_RANGE, gr.CLOSEST_PRUNED],
                         ids=["polyline_closest", "polyline_closest_range", "polyline_closest_pruned"])
def test_host_closest_point_scans_equal_the_oracle(hs, mode):
    gr.check_closest(gr.run_closest(hs, mode), mode)


def test_host_epilines_equal_the_oracle(hs):
    ref, t = gr.reference().epiline, gr.epiline_cases()
    got = gr.run_epiline(hs, t)
    gr.assert_rows_equal("epiline", {"ok": ref.ok, "line": ref.line}, {"ok": got.ok, "line": got.line},
                         {"F": t.F, "valid": t.valid, "xy": t.xy})


def test_broken_tables_are_refused(hs):
    """the input contract is checked before any item runs: -1, outputs untouched"""
    gr.check_broken_tables(hs, lds_on_host=True)
