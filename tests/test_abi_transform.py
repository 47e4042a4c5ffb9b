"""What include/eg3d_transform.h and include/eg3d_host_transform.h promise beyond their signatures and layouts: the codes and
the phrases, the named fields, the callable wrappers, the null-argument refusals of the entry points, and the build
guard's bound on K16. The signatures, layouts, exports and loaded functions of every header are held by tests/test_abi.py;
the tests here that bear those names call it for these two headers and add only what is said above. No GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import forms
import test_abi
from edgegraph3d_amd import _cabi, api, build, host
from edgegraph3d_amd import _cdefs as D
from test_abi import c_layout  # noqa: F401  (the one generated layout program, as a fixture of this module too)

HEADER, HOST_HEADER = "eg3d_transform.h", "eg3d_host_transform.h"


@pytest.mark.parametrize("header", (HEADER, HOST_HEADER), ids=("device", "host"))
def test_table_states_what_the_header_declares(header):
    test_abi.test_table_states_what_the_header_declares(header)


def test_the_headers_state_the_codes_and_what_is_pinned():
    text = open(os.path.join(test_abi.INC, HEADER)).read()   # (header_text drops the preprocessor lines)
    assert re.search(r"#define\s+EG3D_ERR_TRANSFORM_NONFINITE\s+-16\b", text) and api.ERR_TRANSFORM_NONFINITE == -16
    assert re.search(r"#define\s+EG3D_ERR_TRANSFORM_OVERLAP\s+-17\b", text) and api.ERR_TRANSFORM_OVERLAP == -17
    htext = open(os.path.join(test_abi.INC, HOST_HEADER)).read()
    for name, value in (("OK", 0), ("ERR_ARG", -1), ("ERR_FEW", -2), ("ERR_DEGENERATE", -3), ("ERR_NONFINITE", -4), ("ERR_FILE", -5),
                        ("ERR_SHORT", -6)):
        m = re.search(r"#define\s+EG3D_TRANSFORM_%s\s+\(?(-?\d+)\)?" % name, htext)
        assert m and int(m.group(1)) == value, name
        if name != "OK":
            assert getattr(host, "TRANSFORM_" + name) == value
    for phrase in ("UNPINNED", "PINNED", "Eigen::umeyama", "Q16", "has no effect", "never hypot"):
        assert phrase in htext, phrase


def test_the_frozen_tables_are_untouched_and_the_new_ones_disjoint():
    test_abi.test_every_name_has_one_table_and_the_frozen_headers_hold_nothing_of_the_later_ones()
    assert not set(_cabi.EG3D_TRANSFORM) & set(api.EXPORTED_SYMBOLS)


def test_mirrors_have_the_layout_gcc_gives_the_structs(c_layout):  # noqa: F811
    structs = test_abi.header_structs((HEADER, HOST_HEADER))
    assert set(structs) == {"eg3d_transform_stats", "eg3d_similarity_stats"}
    for cname in structs:
        test_abi.test_mirror_has_the_layout_of_the_c_struct(c_layout, cname)
    for f in ("n_points", "n_transformed", "n_nonfinite", "ms_kernel", "ms_copy"):
        assert f in structs["eg3d_transform_stats"], f
    for f in ("scale", "singular", "reflection", "rank_deficient"):
        assert f in structs["eg3d_similarity_stats"], f


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_product_library_exports_the_table(rows):
    test_abi.test_product_library_exports_the_table_and_no_test_hook(rows)


def test_host_library_exports_the_table():
    test_abi.test_host_and_gather_libraries_export_their_tables()
    test_abi.test_loaded_library_declares_every_function_as_its_table_states("host", host.lib)
    for f in ("similarity_fit", "transform_points", "transform_cameras", "camera_errors", "read_camera_poses", "null_cameras"):
        assert callable(getattr(host, f)), f


def test_loaded_library_carries_the_entry_points():
    test_abi.test_loaded_library_declares_every_function_as_its_table_states("eg3d", api.lib)
    for m in ("transform_device", "transform_points"):
        assert callable(getattr(api.Context, m)), m


def test_null_arguments_are_refused():
    L = host.lib()
    T, X = np.eye(4).reshape(16), np.zeros((2, 3), np.float32)
    pT, pX = D.np_ptr(T, C.c_double), D.np_ptr(X, C.c_float)
    xyz = np.zeros((3, 3))
    pxyz = D.np_ptr(xyz, C.c_double)
    assert L.eg3d_host_read_camera_poses(None, 1, pxyz) == -1
    assert L.eg3d_host_read_camera_poses(b"x", 1, None) == -1
    assert L.eg3d_host_read_camera_poses(b"x", -1, pxyz) == -1
    assert L.eg3d_host_similarity_fit(3, None, pxyz, None, pT, None) == -1
    assert L.eg3d_host_similarity_fit(3, pxyz, None, None, pT, None) == -1
    assert L.eg3d_host_similarity_fit(3, pxyz, pxyz, None, None, None) == -1
    small = D.SimilarityStats(struct_size=C.sizeof(D.SimilarityStats) - 4)
    assert L.eg3d_host_similarity_fit(3, pxyz, pxyz, None, pT, C.byref(small)) == -1
    assert L.eg3d_host_transform_points(None, pX, 2, pX) == -1
    assert L.eg3d_host_transform_points(pT, None, 2, pX) == -1
    assert L.eg3d_host_transform_points(pT, pX, 2, None) == -1
    assert L.eg3d_host_transform_points(pT, None, 0, None) == 0
    assert L.eg3d_host_transform_cameras(pT, 1, None, pX, pX, pX, pX) == -1
    assert L.eg3d_host_transform_cameras(None, 0, None, None, None, None, None) == -1
    assert L.eg3d_host_camera_errors(1, pX, None, pxyz, None) == -1
    assert L.eg3d_host_camera_errors(1, None, None, pxyz, C.byref(C.c_float())) == -1
    assert L.eg3d_host_null_cameras(1, None, pX, None) == -1
    assert L.eg3d_host_glm_inverse4(None, pX) == -1 and L.eg3d_host_glm_mul4(pX, None, pX) == -1
    assert L.eg3d_sfm_camera_centres(None, pxyz, None) == -1
    assert L.eg3d_sfm_apply_transform(None, pT, 3) == -1
    s = L.eg3d_sfm_create(2, 64, 48)
    try:
        assert L.eg3d_sfm_apply_transform(s, None, 3) == -1 and L.eg3d_sfm_apply_transform(s, pT, 0) == -1
        assert L.eg3d_sfm_apply_transform(s, pT, 3) == 0
    finally:
        L.eg3d_sfm_destroy(s)
    # the device entry points refuse a null context without touching a device
    st = D.TransformStats(struct_size=C.sizeof(D.TransformStats))
    assert api.lib().eg3d_transform_device(None, None, pT, None, None, C.byref(st)) == -1
    assert api.lib().eg3d_transform_points(None, pT, pX, 2, pX, None) == -1
    tiny = D.TransformStats(struct_size=4)
    assert api.lib().eg3d_transform_points(None, pT, pX, 2, pX, C.byref(tiny)) == -1
    assert b"struct_size" in api.lib().eg3d_last_error()


def test_the_build_guard_holds_k16():
    """No spilled register, no scratch and no LDS in K16, in the bound and in the recorded figures of both libraries; every
    kernel the parent recorded is still recorded."""
    b = build.RESOURCE_BOUNDS["k16_"]
    assert b == {"vgpr_spill_count": 0, "sgpr_spill_count": 0, "private_segment_fixed_size": 0, "group_segment_fixed_size": 0}
    for lib in ("libeg3d", "libeg3d_dlt4x4"):
        rec = json.load(open(os.path.join(build.ROOT, "profiles", "kernel_resources_%s.json" % lib)))
        k16 = {n: r for n, r in rec.items() if "k16_" in n}
        assert list(k16) == ["eg3d::k16_transform"], sorted(k16)
        r = k16["eg3d::k16_transform"]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["agpr_count"] == 0
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0
        assert len([n for n in rec if "k15_" in n]) == 2
