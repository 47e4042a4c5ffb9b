"""What include/eg3d_sets_device.h promises beyond its signatures and layouts (those are held by tests/test_abi.py): the entry
points it was written for, their wrappers on Context, and the build guard's bound on K13. No GPU."""
from edgegraph3d_amd import _cabi, api, build


def test_the_table_names_the_entry_points_and_the_wrappers_are_there():
    assert set(_cabi.EG3D_SETS_DEVICE) >= {"eg3d_upload_polyline_sets", "eg3d_polyline_matches_device",
                                           "eg3d_sets_from_communities_device", "eg3d_polyline_item_samples",
                                           "eg3d_match_polyline_items"}
    for m in ("upload_polyline_sets", "polyline_matches_device", "sets_from_communities_device", "polyline_item_samples",
              "match_polyline_items", "fetch_polyline_sets"):
        assert callable(getattr(api.Context, m)), m


def test_the_build_guard_holds_k13_to_no_spills_no_scratch_no_lds():
    b = build.RESOURCE_BOUNDS["k13_"]
    assert b == {"vgpr_spill_count": 0, "sgpr_spill_count": 0, "private_segment_fixed_size": 0, "group_segment_fixed_size": 0}
