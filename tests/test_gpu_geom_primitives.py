"""-m gpu: the geometry and walk primitives of edgegraph3d_amd/csrc/eg3d_dev_geom.h (and epiline of eg3d_dev_tri.h) ITEM BY
ITEM in their gfx950 compilation: the tables of tests/geom_cases.py, one row per lane and one primitive call per row,
through the TEST-ONLY probe library (tests/probe/libeg3d_probe.so: eg3d_probe_walk / _seg / _cells / _closest / _epiline),
against the reference rows the oracle gave (tests/geom_ref.py) — the rows tests/test_geom_cases.py holds the HOST
compilation of the same header to, without a GPU. Status, segment and the BITS of every coordinate must be equal (NaN equals
NaN, the sign of zero counts), what a primitive leaves untouched included (the outputs start as a sentinel).

What differs between the two compilations on purpose is what this file is for: EG3D_SQRTF / EG3D_SQRT / EG3D_CEILF /
EG3D_FLOORF are builtins on the device, -fhip-fp32-correctly-rounded-divide-sqrt applies there only, the float-to-int
conversion of cell_of is the target's, walk_by_line is also instantiated on an address_space(3) pointer (form 3: no host
build can), and seg_line_cos_gt promises the decisions of the plain expression. Every test re-asserts the coverage
conditions on the rows it compared. (The primitives do not depend on the DLT form: under the suite's two forms the tests
simply run twice.)"""
import ctypes as C
import os

import numpy as np
import pytest

import geom_cases as gc
import geom_ref as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    from edgegraph3d_amd import api
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe", "libeg3d_probe.so")
    assert os.path.exists(path), "tests/probe/libeg3d_probe.so is not built (python -m edgegraph3d_amd.build)"
    L = C.CDLL(path)
    E = gr.bind(L, "eg3d_probe_")
    E.lds_capacity = int(L.eg3d_probe_walk_lds_capacity())
    return E


_WALKS = {}


def _walk(probe, form, tag):
    """(rows compared, result) of one form, run once per pass of the suite (tag: the DLT form of the pass): the forms are also
    compared with each other"""
    if (form, tag) not in _WALKS:
        w = gc.walk_table()
        rows = np.arange(w.n)
        if form == gr.LDS_FORM:   # one polyline per block, staged in LDS: longer ones are left out (none of SIZES is)
            rows = np.flatnonzero(w.row_size <= probe.lds_capacity)
            assert len(rows) == w.n
        _WALKS[(form, tag)] = (rows, gr.run_walk(probe, form, rows))
    return _WALKS[(form, tag)]


@pytest.mark.parametrize("form", sorted(gr.WALK_FORMS), ids=lambda f: gr.WALK_FORMS[f])
def test_walks_equal_the_oracle(probe, form, eg3d_form):
    ref = gr.reference()
    dist = form in gr.DISTANCE_FORMS
    r = ref.walk_dist if dist else ref.walk_line
    rows, got = _walk(probe, form, eg3d_form)
    gr.assert_rows_equal(gr.WALK_FORMS[form], {"status": r.status[rows], "seg": r.seg[rows], "xy": r.xy[rows]},
                         {"status": got.status, "seg": got.seg, "xy": got.xy}, gr.walk_inputs(rows))
    gr.walk_coverage(r if dist else None, None if dist else r, rows)


def test_all_forms_of_a_walk_equal_each_other(probe, eg3d_form):
    """walk_by_distance / walk_by_line are the definitions (eg3d_dev_geom.h): every other form against them, untouched
    outputs included — the address_space(3) instantiation against the global one among them"""
    w = gc.walk_table()
    for base, forms in ((0, gr.DISTANCE_FORMS), (2, gr.LINE_FORMS)):
        rows0, a = _walk(probe, base, eg3d_form)
        assert len(rows0) == w.n
        for form in forms:
            rows, b = _walk(probe, form, eg3d_form)
            gr.assert_rows_equal("%s against %s" % (gr.WALK_FORMS[form], gr.WALK_FORMS[base]),
                                 {"status": a.status[rows], "seg": a.seg[rows], "xy": a.xy[rows]},
                                 {"status": b.status, "seg": b.seg, "xy": b.xy}, gr.walk_inputs(rows))
    untouched = (a.seg == gc.SENT_U32) & (a.xy.view(np.uint32) == np.array([gc.SENT_F32]).view(np.uint32)[0]).all(1)
    assert untouched.sum() >= 1000 and (~untouched).sum() >= 1000


@pytest.mark.parametrize("mode", [gr.SEG_HIT, gr.SEG_GUARDED, gr.SEG_PLDIST, gr.SEG_COS_GT],
                         ids=["seg_line_hit", "seg_line_hit_guarded", "point_line_dist", "seg_line_cos_gt"])
def test_segment_tests_equal_the_oracle(probe, mode):
    ref, t = gr.reference().seg, gc.seg_table()
    inp = {"row": t.rows}
    if mode == gr.SEG_HIT:
        got = gr.run_seg(probe, mode, t.rows)
        gr.assert_rows_equal("seg_line_hit", {"r": ref.hit.r, "hit": ref.hit.o}, {"r": got.r, "hit": got.o}, inp)
    elif mode == gr.SEG_GUARDED:
        got = gr.run_seg(probe, mode, t.rows)
        gr.assert_rows_equal("seg_line_hit_guarded", {"r": ref.guarded.r, "hit": ref.guarded.o}, {"r": got.r, "hit": got.o}, inp)
    elif mode == gr.SEG_PLDIST:
        got = gr.run_seg(probe, mode, t.points)
        gr.assert_rows_equal("point_line_dist", {"d": ref.pldist}, {"d": got.o[:, 0].copy()}, {"row": t.points})
        assert len(t.points) >= 5000 and (np.abs(ref.pldist - 5.0) < 1e-3).sum() >= 100
    else:
        gr.check_cos_gt(ref, gr.run_seg(probe, mode, t.rows), t)
    gr.seg_coverage(ref)   # (every row of the table was compared)


@pytest.mark.parametrize("mode", [gr.CELL_OF, gr.CELL_WINDOW], ids=["cell_of", "cell_window"])
def test_cells_equal_the_oracle(probe, mode):
    """cell_of's (col, row, bx, by) = orc_cell_from_coords' (col, row, on_boundary_row, on_boundary_col): the reference names
    the flag of x "row" and the flag of y "col" (polymatch_ref.cell_from_coords)"""
    ref, t = gr.reference().cells, gc.cell_table()
    got = gr.run_cells(probe, mode)
    if mode == gr.CELL_OF:
        gr.assert_rows_equal("cell_of", {"cell": ref.of}, {"cell": got}, {"row": t.rows})
        gr.cell_coverage(ref)
    else:
        gr.assert_rows_equal("cell_window", {"window": ref.window}, {"window": got}, {"row": t.wrows, "dims": t.wdims})
        gr.window_coverage(ref)


@pytest.mark.parametrize("mode", [gr.CLOSEST_WHOLE, gr.CLOSEST_RANGE, gr.CLOSEST_PRUNED],
                         ids=["polyline_closest", "polyline_closest_range", "polyline_closest_pruned"])
def test_closest_point_scans_equal_the_oracle(probe, mode):
    gr.check_closest(gr.run_closest(probe, mode), mode)


def test_epilines_equal_the_oracle(probe):
    ref, t = gr.reference().epiline, gr.epiline_cases()
    got = gr.run_epiline(probe, t)
    gr.assert_rows_equal("epiline", {"ok": ref.ok, "line": ref.line}, {"ok": got.ok, "line": got.line},
                         {"F": t.F, "valid": t.valid, "xy": t.xy})
    gr.epiline_coverage(ref)


def test_broken_tables_are_refused_before_any_launch(probe):
    """the host side of every entry point checks its table first: -1, nothing launched, outputs untouched"""
    gr.check_broken_tables(probe, lds_on_host=False)
