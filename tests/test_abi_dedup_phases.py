"""The entry points the dedup in phases was written for. The signatures, exports and loaded functions of
include/eg3d_dedup_phases.h, eg3d_host_dedup_phases.h and eg3d_rccl_claims.h, as of every header, are held by
tests/test_abi.py; the tests here that bear those names call it for these three. No GPU, and libeg3d_rccl.so is read with
nm, never loaded."""
import pytest

import forms
import test_abi
from edgegraph3d_amd import _cabi, api, host

NEW_HEADERS = ("eg3d_dedup_phases.h", "eg3d_host_dedup_phases.h", "eg3d_rccl_claims.h")


@pytest.mark.parametrize("header", NEW_HEADERS)
def test_table_states_what_the_header_declares(header):
    test_abi.test_table_states_what_the_header_declares(header)
    assert not test_abi.header_structs((header,))   # scalars and pointers only: these headers define no struct


def test_the_entry_points_the_issue_names_are_there():
    assert set(_cabi.EG3D_DEDUP_PHASES) >= {"eg3d_dedup_claim", "eg3d_dedup_keep", "eg3d_dedup_claims", "eg3d_dedup_merge_claims"}
    assert set(_cabi.EG3D_HOST_DEDUP_PHASES) >= {"eg3d_host_dedup_claim", "eg3d_host_dedup_keep", "eg3d_host_dedup_merge"}
    assert set(_cabi.EG3D_RCCL_CLAIMS) == {"eg3d_allreduce_claims", "eg3d_exscan_points"}


def test_the_frozen_tables_are_untouched_and_the_new_ones_disjoint():
    test_abi.test_every_name_has_one_table_and_the_frozen_headers_hold_nothing_of_the_later_ones()
    assert not set(_cabi.EG3D_DEDUP_PHASES) & set(api.EXPORTED_SYMBOLS)


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_product_library_exports_the_phases(rows):
    test_abi.test_product_library_exports_the_table_and_no_test_hook(rows)


def test_host_and_gather_libraries_export_theirs():
    test_abi.test_host_and_gather_libraries_export_their_tables()
    test_abi.test_loaded_library_declares_every_function_as_its_table_states("host", host.lib)
    test_abi.test_loaded_library_declares_every_function_as_its_table_states("eg3d", api.lib)
