"""The C ABI of the device-resident dedup, without a GPU: Context carries the bindings, and the argument errors that need no
device are refused as such. (The entry points' symbols and the layout of eg3d_dedup_stats are held by tests/test_abi.py.)"""
import ctypes as C

import pytest

import forms
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api


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
