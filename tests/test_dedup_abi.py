"""The C ABI of the device-resident dedup, without a GPU: both product libraries export the entry points, the ctypes
mirror of eg3d_dedup_stats has the layout a C compiler gives the header's struct, and the argument errors that need no
device are refused as such."""
import ctypes as C
import os
import subprocess

import pytest

import forms
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("eg3d_dedup_device", "eg3d_dedup_resident")


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_both_libraries_export_the_entry_points(rows):
    path = forms.lib_path(rows)
    if not os.path.exists(path):
        from edgegraph3d_amd import build
        (build.build_hip if rows == 3 else build.build_hip_dlt4x4)()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in SYMBOLS:
        assert name in exported, (name, path)
        assert name in api.EXPORTED_SYMBOLS


def test_dedup_stats_mirror_matches_the_header(tmp_path):
    fields = [f[0] for f in D.DedupStats._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eg3d.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(eg3d_dedup_stats));\n'
                   + "".join('  printf("%%zu\\n", offsetof(eg3d_dedup_stats, %s));\n' % f for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert nums[0] == C.sizeof(D.DedupStats)
    assert nums[1:] == [getattr(D.DedupStats, f).offset for f in fields]
    assert fields[0] == "struct_size" and D.DedupStats.struct_size.offset == 0 and D.DedupStats.struct_size.size == 4
    for f in ("n_points_in", "n_dedup_kept", "n_gn_inliers", "n_kept", "n_obs_kept", "ms_dedup", "ms_filter", "ms_compact",
              "ms_copy"):
        assert f in fields


def test_context_has_the_bindings():
    for name in ("dedup_device", "dedup_resident"):
        assert callable(getattr(api.Context, name)), name


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_argument_errors_that_need_no_device(rows, monkeypatch):
    monkeypatch.setenv("EG3D_LIB", forms.lib_path(rows))
    monkeypatch.setattr(api, "_LIB", None)
    L = api.lib()
    # a too-small struct_size: refused before the context is looked at, nothing written
    st = D.DedupStats()
    st.struct_size = C.sizeof(D.DedupStats) - 4
    st.n_kept = 12345
    assert L.eg3d_dedup_resident(None, 0, 1, 0, 2.25, 0, -1, None, 0, None, None, C.byref(st)) == -1
    assert b"struct_size" in L.eg3d_last_error() and st.n_kept == 12345
    st.struct_size = C.sizeof(D.DedupStats)
    assert L.eg3d_dedup_resident(None, 0, 1, 0, 2.25, 0, -1, None, 0, None, None, C.byref(st)) == -1
    assert b"struct_size" not in L.eg3d_last_error()
    # index_base + n_points must stay below 2^32 - 1: refused before anything else
    cloud = D.DeviceEdgePoints()
    cloud.n_points, cloud.complete = 1, 1
    for base in (2**32 - 2, 2**32 - 1, 2**32, 2**40, 2**64 - 1):
        assert L.eg3d_dedup_device(None, C.byref(cloud), base, 1, None, None) == -1
        assert b"index_base" in L.eg3d_last_error(), base
    cloud.n_points = 2**32 - 1
    assert L.eg3d_dedup_device(None, C.byref(cloud), 0, 1, None, None) == -1 and b"index_base" in L.eg3d_last_error()
    cloud.n_points = 1
    assert L.eg3d_dedup_device(None, C.byref(cloud), 2**32 - 3, 1, None, None) == -1    # in range: the missing context
    assert b"index_base" not in L.eg3d_last_error()
