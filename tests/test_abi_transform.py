"""What tests/test_abi.py does for the frozen headers, for include/eg3d_transform.h and include/eg3d_host_transform.h: every
function they declare against its row in _cabi.EG3D_TRANSFORM / EG3D_HOST_TRANSFORM, both stats structs against their
ctypes mirrors as gcc lays them out, the tables against the symbols the product libraries and the host library export, the
null-argument refusals of the host entry points, and the build guard's bound on K16. No GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import forms
import test_abi
from edgegraph3d_amd import _cabi, api, build, host
from edgegraph3d_amd import _cdefs as D

HEADER, HOST_HEADER = "eg3d_transform.h", "eg3d_host_transform.h"
MIRRORS = {"eg3d_transform_stats": D.TransformStats, "eg3d_similarity_stats": D.SimilarityStats}
FROZEN = (_cabi.EG3D, _cabi.EG3D_HOST, _cabi.EG3D_RCCL)
OTHERS = (_cabi.EG3D_ACCUMULATE, _cabi.EG3D_HOST_ACCUMULATE, _cabi.EG3D_DEDUP_PHASES, _cabi.EG3D_HOST_DEDUP_PHASES,
          _cabi.EG3D_RCCL_CLAIMS, _cabi.EG3D_REPLAY_MERGE, _cabi.EG3D_HOST_REPLAY_MERGE, _cabi.EG3D_SETS_DEVICE,
          _cabi.EG3D_TRIANGULATE, _cabi.EG3D_HOST_TRIANGULATE, _cabi.EG3D_COLOUR, _cabi.EG3D_HOST_COLOUR)
NEW = (_cabi.EG3D_TRANSFORM, _cabi.EG3D_HOST_TRANSFORM)


def _structs(header):
    out = {}
    for body, name in test_abi.STRUCT.findall(test_abi.header_text(header)):
        decls = [d for d in (x.strip() for x in body.split(";")) if d]
        out[name] = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", piece).group(1) for d in decls for piece in d.split(",")]
    return out


@pytest.mark.parametrize("header,table,count", [(HEADER, _cabi.EG3D_TRANSFORM, 2), (HOST_HEADER, _cabi.EG3D_HOST_TRANSFORM, 10)],
                         ids=("device", "host"))
def test_table_states_what_the_header_declares(header, table, count):
    declared = test_abi.header_functions(header)
    assert set(declared) == set(table), set(declared) ^ set(table)
    assert len(table) == count
    for fn, (ret, params) in declared.items():
        restype, argtypes = table[fn]
        assert (test_abi.ctypes_kind(restype), [test_abi.ctypes_kind(a) for a in argtypes]) == (ret, params), fn


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
    assert [len(t) for t in FROZEN] == [36, 59, 10]
    names = [n for t in FROZEN + OTHERS + NEW for n in t]
    assert len(names) == len(set(names))
    assert sorted(api.TRANSFORM_SYMBOLS) == sorted(_cabi.EG3D_TRANSFORM)
    assert not set(api.TRANSFORM_SYMBOLS) & set(api.EXPORTED_SYMBOLS)
    frozen_text = test_abi.header_text("eg3d.h") + test_abi.header_text("eg3d_host.h")
    for name in list(MIRRORS) + [n for t in NEW for n in t]:   # the frozen headers hold nothing of the new ones
        assert name not in frozen_text, name


def test_mirrors_have_the_layout_gcc_gives_the_structs(tmp_path):
    structs = dict(_structs(HEADER), **_structs(HOST_HEADER))
    assert set(structs) == set(MIRRORS), set(structs) ^ set(MIRRORS)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, '#include "%s"' % HOST_HEADER, "int main(void) {"]
    for s, members in structs.items():
        lines.append('  printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['  printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, m, s, m, s, m) for m in members]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", test_abi.INC, str(tmp_path / "layout.c"), "-o", exe])
    got = {}
    for w in (l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()):
        if w[0] == "S":
            got[w[1]] = {"size": int(w[2]), "fields": []}
        else:
            got[w[1]]["fields"].append([w[2], int(w[3]), int(w[4])])
    for cname, mirror in MIRRORS.items():
        assert got[cname]["size"] == C.sizeof(mirror), cname
        assert got[cname]["fields"] == [[f[0], getattr(mirror, f[0]).offset, getattr(mirror, f[0]).size] for f in mirror._fields_], cname
        assert got[cname]["fields"][0] == ["struct_size", 0, 4], cname   # new structs carry their size first
    for f in ("n_points", "n_transformed", "n_nonfinite", "ms_kernel", "ms_copy"):
        assert f in structs["eg3d_transform_stats"], f
    for f in ("scale", "singular", "reflection", "rank_deficient"):
        assert f in structs["eg3d_similarity_stats"], f


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_product_library_exports_the_table(rows):
    path = forms.lib_path(rows)
    if not os.path.exists(path):
        (build.build_hip if rows == 3 else build.build_hip_dlt4x4)()
    syms = test_abi.exported(path)
    assert not set(_cabi.EG3D_TRANSFORM) - syms, set(_cabi.EG3D_TRANSFORM) - syms
    assert not set(_cabi.EG3D_HOST_TRANSFORM) & syms   # (the product library does not carry the host statement)


def test_host_library_exports_the_table():
    syms = test_abi.exported(build.build_host())
    assert not set(_cabi.EG3D_HOST_TRANSFORM) - syms
    for name in _cabi.EG3D_HOST_TRANSFORM:
        assert _cabi.EG3D_HOST_TRANSFORM[name][1] == getattr(host.lib(), name).argtypes
    for f in ("similarity_fit", "transform_points", "transform_cameras", "camera_errors", "read_camera_poses", "null_cameras"):
        assert callable(getattr(host, f)), f


def test_loaded_library_carries_the_entry_points():
    for name in _cabi.EG3D_TRANSFORM:   # (the C-ABI library loads without a GPU)
        assert hasattr(api.lib(), name), name
        assert _cabi.EG3D_TRANSFORM[name][1] == getattr(api.lib(), name).argtypes
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
