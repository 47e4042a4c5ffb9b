"""What tests/test_abi.py does for the three frozen headers, for the three headers of the dedup in phases: every function
include/eg3d_dedup_phases.h, eg3d_host_dedup_phases.h and eg3d_rccl_claims.h declare against its row in
edgegraph3d_amd/_cabi.py, and the tables against the symbols the built libraries export. No GPU, and libeg3d_rccl.so is
read with nm, never loaded."""
import os

import pytest

import forms
import test_abi
from edgegraph3d_amd import _cabi, api, build, host

NEW_TABLES = {"eg3d_dedup_phases.h": _cabi.EG3D_DEDUP_PHASES, "eg3d_host_dedup_phases.h": _cabi.EG3D_HOST_DEDUP_PHASES,
              "eg3d_rccl_claims.h": _cabi.EG3D_RCCL_CLAIMS}
FROZEN = (_cabi.EG3D, _cabi.EG3D_HOST, _cabi.EG3D_RCCL, _cabi.EG3D_ACCUMULATE, _cabi.EG3D_HOST_ACCUMULATE)


@pytest.mark.parametrize("header", sorted(NEW_TABLES))
def test_table_states_what_the_header_declares(header):
    declared, table = test_abi.header_functions(header), NEW_TABLES[header]
    assert set(declared) == set(table), set(declared) ^ set(table)
    for fn, (ret, params) in declared.items():
        restype, argtypes = table[fn]
        assert (test_abi.ctypes_kind(restype), [test_abi.ctypes_kind(a) for a in argtypes]) == (ret, params), fn
    assert not [n for n in table if "probe" in n or "internal" in n]
    # scalars and pointers only: the new headers define no struct
    assert not test_abi.STRUCT.findall(test_abi.header_text(header))


def test_the_entry_points_the_issue_names_are_there():
    assert set(_cabi.EG3D_DEDUP_PHASES) >= {"eg3d_dedup_claim", "eg3d_dedup_keep", "eg3d_dedup_claims", "eg3d_dedup_merge_claims"}
    assert set(_cabi.EG3D_HOST_DEDUP_PHASES) >= {"eg3d_host_dedup_claim", "eg3d_host_dedup_keep", "eg3d_host_dedup_merge"}
    assert set(_cabi.EG3D_RCCL_CLAIMS) == {"eg3d_allreduce_claims", "eg3d_exscan_points"}


def test_the_frozen_tables_are_untouched_and_the_new_ones_disjoint():
    assert [len(t) for t in FROZEN] == [36, 59, 10, 2, 5]
    names = [n for t in FROZEN + tuple(NEW_TABLES.values()) for n in t]
    assert len(names) == len(set(names))
    assert sorted(api.DEDUP_PHASES_SYMBOLS) == sorted(_cabi.EG3D_DEDUP_PHASES)
    assert not set(api.DEDUP_PHASES_SYMBOLS) & set(api.EXPORTED_SYMBOLS)


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_product_library_exports_the_phases(rows):
    path = forms.lib_path(rows)
    if not os.path.exists(path):
        (build.build_hip if rows == 3 else build.build_hip_dlt4x4)()
    syms = test_abi.exported(path)
    assert not set(_cabi.EG3D_DEDUP_PHASES) - syms, set(_cabi.EG3D_DEDUP_PHASES) - syms
    assert not set(_cabi.EG3D_HOST_DEDUP_PHASES) & syms   # (the host statement lives in libeg3d_host.so alone)


def test_host_and_gather_libraries_export_theirs():
    assert not set(_cabi.EG3D_HOST_DEDUP_PHASES) - test_abi.exported(build.HOST_LIB)
    assert not set(_cabi.EG3D_RCCL_CLAIMS) - test_abi.exported(build.RCCL_LIB)
    for name in _cabi.EG3D_HOST_DEDUP_PHASES:
        assert hasattr(host.lib(), name), name
    for name in _cabi.EG3D_DEDUP_PHASES:   # (the C-ABI library loads without a GPU)
        assert hasattr(api.lib(), name), name
        assert _cabi.EG3D_DEDUP_PHASES[name][1] == getattr(api.lib(), name).argtypes
