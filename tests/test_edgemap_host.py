"""K19 without a GPU: the host statement of the edge maps (eg3d_host_edge_maps) against the numpy restatement
(tests/edgemap_ref.py), bit for bit, on every case of tests/edgemap_cases.py and on one full 1600 x 1200 rendered view;
the 1-bit PNG writer through both readers; plg_views_from_masks against plg_from_mask; every refusal of E7 with
canary-filled outputs, in both libraries (the device library decides them before it touches a device); the build guard's
row and the recorded k19_ kernels against the kernels the source defines."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import edgemap_cases as ec
import edgemap_ref as R
import png_util
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, build, host


@pytest.mark.parametrize("name", ec.names())
def test_host_statement_equals_the_restatement(name):
    c = ec.case(name)
    want_masks, want = ec.expected(name)
    masks, stats = host.edge_maps(c["images"], **ec.params(c))
    assert len(masks) == len(want_masks)
    for m, w in zip(masks, want_masks):
        assert m.dtype == np.uint8 and m.shape == w.shape and np.array_equal(m, w)
    for k in ec.COUNTS:
        assert stats[k] == want[k], k


def test_host_statement_equals_the_restatement_on_a_full_view():
    im = ec.full_view()
    assert im.shape == (1200, 1600, 3)
    masks, stats = host.edge_maps([im], 40, 100)
    want_masks, want = R.edge_maps([im], 40, 100)
    assert np.array_equal(masks[0], want_masks[0])
    for k in ec.COUNTS:
        assert stats[k] == want[k], k
    assert 0 < stats["n_strong"] < stats["n_candidates"] and stats["n_strong"] < stats["n_edges"] < stats["n_candidates"]
    # the edges are thin: no 3 x 3 block is fully set
    from scipy import ndimage
    assert not ndimage.binary_erosion(masks[0], structure=np.ones((3, 3))).any()


def test_the_rules_hold_on_hand_computed_pixels():
    """E1's rounding, E2's fold and E4's two forms on values small enough to do by hand."""
    assert [int(R.grey(np.array([p], np.uint8))[0]) for p in ((255, 255, 255), (0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255), (1, 1, 1))] == [
        255, 0, 76, 150, 29, 1]
    assert R.reflect101(np.arange(-5, 8), 4).tolist() == [1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1]
    assert R.reflect101(np.arange(-3, 4), 1).tolist() == [0] * 7 and R.reflect101(np.arange(-3, 5), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    # a vertical step of 10 grey levels: |gx| = 40 on the two columns beside it; the left one is kept (m > left, m >= right)
    im = ec.rgb_of(np.where(np.arange(8)[None, :] >= 4, 110, 100) * np.ones((5, 1), int))
    for l2, lo, hi in ((False, 39, 39), (True, 39, 39), (False, 40, 40), (True, 40, 40)):
        masks, stats = host.edge_maps([im], lo, hi, 0, l2)
        assert masks[0][:, 3].all() == (lo < 40) and not masks[0][:, [0, 1, 2, 4, 5, 6, 7]].any(), (l2, lo)


def test_png_writer_round_trips_through_both_readers(tmp_path):
    rng = np.random.default_rng(3)
    masks = [rng.integers(0, 2, (h, w), dtype=np.uint8) for h, w in ((1, 1), (3, 7), (5, 8), (4, 9), (66, 130))]
    masks.append(ec.expected("golden_crop")[0][0])
    masks.append(np.zeros((6, 17), np.uint8))
    masks.append(np.full((6, 17), 7, np.uint8))      # any non-zero value is an edge
    for i, m in enumerate(masks):
        path = str(tmp_path / ("m%d.png" % i))
        host.write_png_mask(path, m)
        want = (m != 0).astype(np.uint8)
        assert np.array_equal(host.png_edge_mask(path), want), i
        assert np.array_equal(np.asarray(png_util.read_png_edge_mask(path)), want), i
        data = open(path, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[24:29] == bytes([1, 0, 0, 0, 0])       # 1 bit, grey, no interlace
    L = host.lib()
    one = np.ones((2, 2), np.uint8)
    assert L.eg3d_host_png_write_mask(None, D.np_ptr(one, C.c_uint8), 2, 2) == -1
    assert L.eg3d_host_png_write_mask(str(tmp_path / "x.png").encode(), None, 2, 2) == -1
    assert L.eg3d_host_png_write_mask(str(tmp_path / "x.png").encode(), D.np_ptr(one, C.c_uint8), 0, 2) == -1
    assert L.eg3d_host_png_write_mask(str(tmp_path / "x.png").encode(), D.np_ptr(one, C.c_uint8), 2, 16385) == -1
    assert not os.path.exists(str(tmp_path / "x.png"))
    assert L.eg3d_host_png_write_mask(str(tmp_path / "no_such_dir" / "x.png").encode(), D.np_ptr(one, C.c_uint8), 2, 2) == -2
    assert b"eg3d_host_png_write_mask" in L.eg3d_host_edgemap_last_error()


def test_plg_views_from_masks_equals_plg_from_mask_view_by_view():
    masks = [ec.expected(n)[0][0] for n in ("golden_crop", "serpentine", "scene_p0_l1", "constant", "size_1x1_p0", "golden_crop_l2_p0")]
    assert sum(int(m.sum()) for m in masks) > 3000
    got = host.plg_views_from_masks(masks)
    assert len(got) == len(masks)
    for g, m in zip(got, masks):
        want = host.plg_from_mask(m)
        assert set(g) == set(want)
        for k in want:
            assert np.array_equal(g[k], want[k]), k
    assert got[0]["n_polylines"] > 20 and got[3]["n_polylines"] == 0
    assert host.plg_views_from_masks([]) == []
    L = host.lib()
    v = (D.PlgView * 1)()
    w = np.array([4], np.int32)
    assert L.eg3d_host_plg_build_views_from_masks(None, 1, D.np_ptr(w, C.c_int32), D.np_ptr(w, C.c_int32), v) == -1
    assert L.eg3d_host_plg_build_views_from_masks(None, -1, None, None, None) == -1


# ---- E7 ------------------------------------------------------------------------------------------------------------------
CANARY = 0xA5


def _call(fn, n_views=1, w=(5,), h=(4,), low=10, high=20, passes=1, l2=0, null=(), params_size=None, stats_size=None):
    """One native call on canary-filled masks and stats; returns (rc, every output byte is still the canary)."""
    n = len(w)
    imgs = [np.zeros((max(hh, 1), max(ww, 1), 3), np.uint8) for ww, hh in zip(w, h)]
    masks = [np.full((max(hh, 1), max(ww, 1)), CANARY, np.uint8) for ww, hh in zip(w, h)]
    wa, ha = np.array(w, np.int32), np.array(h, np.int32)
    in_p = (D.u8p * n)(*[None if ("rgb", v) in null else D.np_ptr(imgs[v], C.c_uint8) for v in range(n)])
    out_p = (D.u8p * n)(*[None if ("mask", v) in null else D.np_ptr(masks[v], C.c_uint8) for v in range(n)])
    params = D.EdgemapParams(struct_size=C.sizeof(D.EdgemapParams) if params_size is None else params_size, low=low, high=high,
                             smooth_passes=passes, l2=l2)
    st = D.EdgemapStats()
    C.memset(C.byref(st), CANARY, C.sizeof(st))
    st.struct_size = C.sizeof(D.EdgemapStats) if stats_size is None else stats_size
    rc = fn(n_views, None if "width" in null else D.np_ptr(wa, C.c_int32), None if "height" in null else D.np_ptr(ha, C.c_int32),
            None if "rgb" in null else in_p, None if "params" in null else C.byref(params), None if "masks" in null else out_p,
            None if "stats" in null else C.byref(st))
    raw = bytes(st)[4:]
    return rc, all((m == CANARY).all() for m in masks) and raw == bytes([CANARY]) * len(raw)


REFUSALS = {
    "null_width": dict(null=("width",)), "null_height": dict(null=("height",)), "null_rgb": dict(null=("rgb",)),
    "null_masks": dict(null=("masks",)), "null_params": dict(null=("params",)),
    "null_image_of_a_view": dict(w=(5, 6), h=(4, 3), n_views=2, null=(("rgb", 1),)),
    "null_mask_of_a_view": dict(w=(5, 6), h=(4, 3), n_views=2, null=(("mask", 0),)),
    "no_views": dict(n_views=0), "negative_views": dict(n_views=-3),
    "zero_width": dict(w=(0,)), "zero_height": dict(h=(0,)), "negative_width": dict(w=(-5,)),
    "width_above_16384": dict(w=(16385,), h=(1,)), "height_above_16384": dict(w=(1,), h=(16385,)),
    "bad_second_view": dict(w=(5, 0), h=(4, 3), n_views=2),
    "negative_low": dict(low=-1), "low_above_high": dict(low=21, high=20), "high_above_65535": dict(high=65536),
    "negative_passes": dict(passes=-1), "five_passes": dict(passes=5), "l2_of_two": dict(l2=2),
    "short_params": dict(params_size=8), "short_stats": dict(stats_size=8),
}


@pytest.mark.parametrize("why", list(REFUSALS))
@pytest.mark.parametrize("library", ["host", "device"])
def test_every_refusal_leaves_the_outputs_untouched(library, why):
    """The device library refuses all of these before it asks for a device, so this needs none."""
    if library == "host":
        fn, err = host.lib().eg3d_host_edge_maps, host.lib().eg3d_host_edgemap_last_error
    else:
        L = api.lib()
        fn, err = (lambda *a: L.eg3d_edge_maps(0, *a)), L.eg3d_last_error
    rc, untouched = _call(fn, **REFUSALS[why])
    assert rc == -1 and untouched
    assert (b"eg3d_host_edge_maps: " if library == "host" else b"eg3d_edge_maps: ") in err()


def test_what_is_no_refusal_is_accepted_by_the_host_statement():
    fn = host.lib().eg3d_host_edge_maps
    for ok in (dict(), dict(null=("stats",)), dict(low=0, high=0, passes=0), dict(low=65535, high=65535, passes=4, l2=1),
               dict(params_size=C.sizeof(D.EdgemapParams) + 8, stats_size=C.sizeof(D.EdgemapStats) + 8), dict(w=(1,), h=(1,))):
        rc, untouched = _call(fn, **ok)
        assert rc == 0 and not untouched, ok
    with pytest.raises(ValueError):
        host.edge_maps([np.zeros((4, 4), np.uint8)], 1, 2)
    with pytest.raises(RuntimeError, match="n_views"):
        host.edge_maps([], 1, 2)


# ---- the build guard ---------------------------------------------------------------------------------------------------------
def _source_kernels():
    text = open(os.path.join(build.CSRC_DIR, "eg3d_k19_edgemap.hip")).read()
    return {"eg3d::" + m for m in re.findall(r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(k19_\w+)\s*\(", text)}


def test_the_build_guard_holds_k19():
    b = build.RESOURCE_BOUNDS["k19_"]
    assert b["vgpr_spill_count"] == 0 and b["sgpr_spill_count"] == 0 and b["private_segment_fixed_size"] == 0
    want = _source_kernels()
    assert want == {"eg3d::k19_" + k for k in ("smooth", "classify", "hysteresis", "mask")}
    for lib in ("libeg3d", "libeg3d_dlt4x4"):
        rec = json.load(open(os.path.join(build.ROOT, "profiles", "kernel_resources_%s.json" % lib)))
        k19 = {n: r for n, r in rec.items() if "k19_" in n}
        assert {re.sub(r"^void ", "", n).split("(")[0].split("<")[0] for n in k19} == want, sorted(k19)
        assert len(k19) == 6                        # smooth and classify once per source form
        for n, r in k19.items():
            assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, n
            # LDS as the build reports it: the bound of the kernel's own row, or of the "k19_" row for the largest (classify)
            rows = [v["group_segment_fixed_size"] for k, v in build.RESOURCE_BOUNDS.items() if k.startswith("k19_") and k in n]
            assert r["group_segment_fixed_size"] == min(rows), n
        assert len([n for n in rec if "k18_" in n]) == 10 and len([n for n in rec if "k17_" in n]) == 12


def test_the_cases_are_built_against_the_kernels_tile():
    text = open(os.path.join(build.CSRC_DIR, "eg3d_k19_edgemap.h")).read()
    assert int(re.search(r"#define K19_TILE (\d+)", text).group(1)) == ec.TILE
    core = open(os.path.join(build.CSRC_DIR, "eg3d_edgemap_core.h")).read()
    assert "EG3D_HD" in core
    for f in (os.path.join(build.CSRC_DIR, "eg3d_k19_edgemap.h"), os.path.join(build.HOST_DIR, "edgemap.cpp")):
        assert '#include "eg3d_edgemap_core.h"' in open(f).read(), f
