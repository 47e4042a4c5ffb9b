"""-m gpu: K19, the edge maps of the source images on the device (include/eg3d/edgemap.hh) against the sequential statement
eg3d_host_edge_maps, bit for bit — every mask, every count —, once per product library:
  * every case of tests/edgemap_cases.py on its own, and again as views in the middle of a larger call;
  * an input without any edge (a constant image: the empty mask) and the 1 x 1 image;
  * the serpentine needs rounds of the propagation, and the diagonal across a tile corner is crossed;
  * the masks feed host.plg_from_mask;
  * the refusals return before the device is asked for anything, the outputs untouched.
The host statement itself is held to the numpy restatement in tests/test_edgemap_host.py; what it gives for a case is
computed once here. No test provokes a fault: every refusal is decided on the host."""
import numpy as np
import pytest

import edgemap_cases as ec
import test_edgemap_host as eh
from edgegraph3d_amd import api, host

pytestmark = pytest.mark.gpu
_WANT = {}     # case name -> the host statement's (masks, stats), computed once
_FILL = {}     # parameters -> the host statement's masks of the fillers


def _want(name):
    if name not in _WANT:
        c = ec.case(name)
        _WANT[name] = host.edge_maps(c["images"], **ec.params(c))
    return _WANT[name]


def _same(got, want):
    masks, stats = got
    wmasks, wstats = want
    assert len(masks) == len(wmasks)
    for m, w in zip(masks, wmasks):
        assert m.dtype == np.uint8 and m.shape == w.shape and np.array_equal(m, w)
    for k in ec.COUNTS:
        assert stats[k] == wstats[k], k


@pytest.mark.parametrize("name", ec.names())
def test_device_equals_the_host_statement(name):
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    c = ec.case(name)
    got = api.edge_maps(c["images"], **ec.params(c))
    _same(got, _want(name))
    for k in ("ms_upload", "ms_kernel", "ms_hysteresis", "ms_copy"):
        assert got[1][k] >= 0.0


@pytest.mark.parametrize("name", ec.names())
def test_device_equals_the_host_statement_inside_a_larger_call(name):
    c = ec.case(name)
    p = ec.params(c)
    key = tuple(sorted(p.items()))
    if key not in _FILL:
        _FILL[key] = host.edge_maps(list(ec.FILLERS), **p)[0]
    n = len(c["images"])
    masks, stats = api.edge_maps([ec.FILLERS[0]] + c["images"] + [ec.FILLERS[1]], **p)
    assert len(masks) == n + 2 and stats["n_views"] == n + 2
    want = _want(name)[0]
    for m, w in zip(masks[1:-1], want):
        assert np.array_equal(m, w)
    assert np.array_equal(masks[0], _FILL[key][0]) and np.array_equal(masks[-1], _FILL[key][1])
    assert stats["n_edges"] == sum(int(m.sum()) for m in list(want) + list(_FILL[key]))


def test_an_input_without_edges_and_the_smallest_input_pass():
    masks, stats = api.edge_maps([np.full((20, 23, 3), 137, np.uint8)], 0, 0)
    assert not masks[0].any() and stats["n_candidates"] == stats["n_edges"] == 0 and stats["hysteresis_rounds"] == 0
    for value in (0, 255):
        masks, stats = api.edge_maps([np.full((1, 1, 3), value, np.uint8)], 0, 65535, smooth_passes=4, l2=True)
        assert masks[0].shape == (1, 1) and not masks[0].any() and stats["n_pixels"] == 1


def test_the_serpentine_takes_rounds_and_the_tile_corner_is_crossed():
    c = ec.case("serpentine")
    masks, stats = api.edge_maps(c["images"], **ec.params(c))
    assert stats["hysteresis_rounds"] >= 1
    assert stats["n_strong"] == 1 and stats["n_edges"] == stats["n_candidates"] == int(masks[0].sum()) > 1000
    c = ec.case("diagonal_across_tile_corner")
    masks, stats = api.edge_maps(c["images"], **ec.params(c))
    a, b = ec.TILE - 1, ec.TILE
    assert masks[0][a, a] and masks[0][b, b] and not masks[0][a, b] and not masks[0][b, a]
    assert stats["n_edges"] == stats["n_candidates"] and masks[0][b + 5:, b].any()      # the part beyond the corner is kept
    c = ec.case("weak_only")
    masks, stats = api.edge_maps(c["images"], **ec.params(c))
    assert stats["n_candidates"] > 0 and stats["n_strong"] == 0 and not masks[0].any()


def test_the_masks_feed_the_polyline_builder():
    c = ec.case("golden_crop")
    masks, _ = api.edge_maps(c["images"], **ec.params(c))
    g = host.plg_from_mask(masks[0])
    want = host.plg_from_mask(_want("golden_crop")[0][0])
    assert g["n_polylines"] == want["n_polylines"] > 20 and np.array_equal(g["vtx_xy"], want["vtx_xy"])
    views = host.plg_views_from_masks(masks)
    assert np.array_equal(views[0]["pl_vtx_off"], want["pl_vtx_off"])


@pytest.mark.parametrize("why", list(eh.REFUSALS))
def test_the_refusals_return_without_a_launch(why):
    L = api.lib()
    rc, untouched = eh._call(lambda *a: L.eg3d_edge_maps(0, *a), **eh.REFUSALS[why])
    assert rc == -1 and untouched and b"eg3d_edge_maps: " in L.eg3d_last_error()


def test_a_device_that_does_not_exist_is_refused():
    L = api.lib()
    rc, untouched = eh._call(lambda *a: L.eg3d_edge_maps(api.device_count(), *a))
    assert rc == -1 and untouched and b"device index" in L.eg3d_last_error()
    rc, untouched = eh._call(lambda *a: L.eg3d_edge_maps(0, *a))
    assert rc == 0 and not untouched
