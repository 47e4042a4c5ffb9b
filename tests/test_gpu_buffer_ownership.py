"""-m gpu: who frees what. Every device allocation of the library is counted (eg3d_test_live_device_bytes, tests only):
each case notes the count, uses contexts the way a caller does, and asserts that the count rose in between and is EXACTLY
back once the last context is gone — a work buffer nobody releases, a scene or seed buffer released twice or by the wrong
owner, or a temporary that outlives its call shows as a difference. The scene is the tiny generated one (host.Synth(0): 4
views, 8 curves, 40 seeds)."""
import ctypes as C

import numpy as np
import pytest

from edgegraph3d_amd import api, host

pytestmark = pytest.mark.gpu

CLOUD = ("X", "obs_off", "obs_view", "obs_pl", "obs_seg", "obs_xy", "key")
GRAPH = ("node_view", "node_pl", "adj_off", "adj_node", "adj_w", "point_weight", "cp_off", "cp_view", "cp_pl", "cr_off", "cr_point")


def _live():
    f = api.lib().eg3d_test_live_device_bytes
    f.restype, f.argtypes = C.c_int64, []
    return int(f())


@pytest.fixture
def tiny():
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return host.Synth(0)


def _same(a, b, keys):
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _every_stage(ctx, s):
    """Every stage once on `ctx`; returns the cloud of the match and the compatibility graph."""
    ctx.upload_seeds(s.seeds)
    n = s.n_seeds
    cloud = ctx.match_resident(0, n)   # (a context's first host call runs on the context alone: the device view is whole)
    assert cloud["n_points"] > 0
    _, _, fs = ctx.filter_resident()
    assert fs["n_points_in"] == cloud["n_points"]
    _, _, ds = ctx.dedup_resident()
    assert ds["n_points_in"] == cloud["n_points"]
    graph3d, _, rs = ctx.replay_device()
    assert rs["n_nodes"] > 0
    pm = ctx.match_polylines_closeness(None, 0, n)
    assert pm["stats"]["n_entries"] > 0 and pm["n_sets"] > 0
    ctx.grid(0, 2)   # the 10 px map exists (and belongs to the grids the context shares with its clones)
    sg = ctx.similarity_graph(None, 0, n)
    assert sg["n_nodes"] > 0 and sg["stats"]["n_pair_instances"] >= 3
    cm = ctx.communities(sg)
    assert cm["n_communities"] > 0
    return cloud, sg


def test_every_stage_in_one_context(tiny):
    before = _live()
    ctx = api.Context(tiny.scene)
    scene_only = _live()
    assert scene_only > before
    _every_stage(ctx, tiny)
    assert _live() > scene_only
    ctx.close()
    assert _live() == before


def test_chunked_clique_expansion_grows_and_keeps(tiny, monkeypatch):
    """EG3D_SIMGRAPH_PAIR_BUDGET cuts the pair instances into three chunks or more: the distinct edges so far are kept
    while their buffer grows (ensure_keep). The graph is the one of the default budget."""
    before = _live()
    ctx = api.Context(tiny.scene)
    _, want = _every_stage(ctx, tiny)
    ctx.close()
    assert _live() == before
    n_inst, n_edges = want["stats"]["n_pair_instances"], want["stats"]["n_edges"]
    budget = max(1, min(n_inst // 3, n_edges // 2))
    # The first chunk finds no distinct key to keep and sizes the key buffer for itself: 8 B x budget + a quarter, at least
    # 256 B. The chunk that completes the distinct list needs 8 B x (at least n_edges) — more than that block, so a later
    # chunk, which has keys to keep, grows the buffer around them.
    assert 8 * n_edges > max(10 * budget, 256)
    monkeypatch.setenv("EG3D_SIMGRAPH_PAIR_BUDGET", str(budget))   # (read when a context is created)
    ctx = api.Context(tiny.scene)
    monkeypatch.delenv("EG3D_SIMGRAPH_PAIR_BUDGET")
    _, got = _every_stage(ctx, tiny)
    assert got["stats"]["n_chunks"] >= 3 and want["stats"]["n_chunks"] == 1
    _same(got, want, GRAPH)
    assert got["n_nodes"] == want["n_nodes"]
    assert _live() > before
    ctx.close()
    assert _live() == before


@pytest.mark.parametrize("parent_first", [True, False])
def test_three_lanes_a_clone_and_either_order_of_destruction(tiny, parent_first):
    """A parent and a clone share the scene and the seeds; each cuts its calls into three units on three lanes (internal
    clones with their own work buffers). Whichever goes first, the other still matches correctly, and the shared buffers
    go with the last of them."""
    before = _live()
    parent = api.Context(tiny.scene)
    parent.upload_seeds(tiny.seeds)
    n = tiny.n_seeds
    parent.set_pipelining(1, 0)
    want = parent.match_resident(0, n)
    assert want["n_points"] > 0
    clone = parent.clone()
    for c in (parent, clone):
        c.set_pipelining(3, 3)
        _same(c.match_resident(0, n), want, CLOUD)
    both = _live()
    assert both > before
    first, last = (parent, clone) if parent_first else (clone, parent)
    first.close()
    assert before < _live() < both
    _same(last.match_resident(0, n), want, CLOUD)
    last.close()
    assert _live() == before


def test_seeds_uploaded_twice_with_different_sizes(tiny):
    """The first set's buffers go away with their last owner — here the context itself, at the second upload."""
    before = _live()
    off, view, xy = tiny.seeds_np()
    n = len(off) - 1
    half = host.SeedsArrays(off[:n // 2 + 1].copy(), view[:off[n // 2]].copy(), xy[:off[n // 2]].copy())
    ctx = api.Context(tiny.scene)
    scene_only = _live()
    ctx.upload_seeds(C.byref(half.c))
    with_half = _live()
    ctx.upload_seeds(tiny.seeds)
    with_all = _live()
    assert scene_only < with_half <= with_all
    ctx.upload_seeds(C.byref(half.c))
    assert _live() == with_half
    part = ctx.match_resident(0, n // 2)
    ctx.upload_seeds(tiny.seeds)
    whole = ctx.match_resident(0, n)
    assert 0 < part["n_points"] <= whole["n_points"]
    assert _live() > with_all
    ctx.close()
    assert _live() == before


def test_creation_that_fails_after_the_scene_was_uploaded(tiny, monkeypatch):
    """The product libraries are built without the lane-per-chain engine and refuse EG3D_K3B_ENGINE=1 at eg3d_create —
    after the scene was uploaded and its grids were built (eg3d_api.hip): the scene buffers still belong to the half-made
    context, which frees them exactly once."""
    before = _live()
    monkeypatch.setenv("EG3D_K3B_ENGINE", "1")
    with pytest.raises(api.Eg3dError) as ei:
        api.Context(tiny.scene)
    assert "EG3D_K3B_ENGINE" in str(ei.value)
    assert _live() == before
    monkeypatch.delenv("EG3D_K3B_ENGINE")
    ctx = api.Context(tiny.scene)   # (... and the next creation is whole)
    assert _live() > before
    ctx.close()
    assert _live() == before
