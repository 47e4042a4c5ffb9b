"""The device-resident filter stage, without a GPU: Context carries the bindings. (The entry points' symbols and the layout
of eg3d_filter_stats are held by tests/test_abi.py.)"""
from edgegraph3d_amd import api


def test_context_has_the_bindings():
    for name in ("gn_filter_device", "compact_device", "filter_resident", "device_alloc", "upload"):
        assert callable(getattr(api.Context, name)), name
