"""-m gpu: who frees what. Every device allocation of the library is counted (eg3d_test_live_device_bytes, tests only):
each case notes the count, uses contexts the way a caller does (a context, its clones, their clones and the lanes of a call
share one scene and, until the next upload, one set of seeds), and asserts that the count rose in between and is EXACTLY
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


# ---- what a context shares, what it learns, and who gets it ------------------------------------------------------------------
# The retries of the expand stage are forced from a context's first call until it has learned the sizes (test_gpu_stage_b_retries.py
# has each of them alone); who STARTS from what was learned shows in the trace. EG3D_ARENA_CAP0 is left out: it applies to every call.
FORCED = (("EG3D_HITS_CAP0", "1"), ("EG3D_CHAIN_CAP0", "8"), ("EG3D_POOL_CAP0", "64"), ("EG3D_STAGE_CAP0", "1"),
          ("EG3D_TRACE_ARENA", "1"))
RETRIES = ("K2 runs again", "relaunching", "staging area")
_CHAINS = {}


def _chains(rows):
    """host.Synth(1) (the smallest scene with chains) and its cloud from a context no knob touches, uncut: once per DLT
    form, shared read-only. Call it BEFORE setting a knob."""
    if rows not in _CHAINS:
        s = host.Synth(1)
        ctx = api.Context(s.scene)
        ctx.upload_seeds(s.seeds)
        ctx.set_pipelining(1, 0)
        _CHAINS[rows] = (s, ctx.match_resident(0, s.n_seeds))
        ctx.close()
        assert _CHAINS[rows][1]["n_chains"] > 0
    return _CHAINS[rows]


def _traced(capfd, ctx, n):
    """The cloud of one uncut call and which of the three retries its trace names."""
    capfd.readouterr()
    cloud = ctx.match_resident(0, n)
    err = capfd.readouterr().err
    return cloud, {m for m in RETRIES if m in err}


def test_a_clone_starts_from_what_its_parent_has_learned_and_an_earlier_clone_does_not(eg3d_form, monkeypatch, capfd):
    s, want = _chains(eg3d_form)
    before = _live()
    for k, v in FORCED:
        monkeypatch.setenv(k, v)
    parent = api.Context(s.scene)
    parent.upload_seeds(s.seeds)
    parent.set_pipelining(1, 0)
    early = parent.clone()                      # (made while the parent has learned nothing)
    cloud, retried = _traced(capfd, parent, s.n_seeds)
    assert retried == set(RETRIES)
    _same(cloud, want, CLOUD)
    late = parent.clone()
    cloud, retried = _traced(capfd, late, s.n_seeds)
    assert retried == set()
    _same(cloud, want, CLOUD)
    cloud, retried = _traced(capfd, early, s.n_seeds)
    assert retried == set(RETRIES)
    _same(cloud, want, CLOUD)
    for c in (parent, early, late):
        c.close()
    assert _live() == before


def test_lanes_give_back_what_they_learned(eg3d_form, monkeypatch, capfd):
    """Five units on three lanes, each lane starting from nothing; the uncut call behind them on the same context runs
    on the context alone and repeats nothing: the slice and hit capacities came back from the lanes, and the staging area
    is the context's own (lane 0 is the context itself)."""
    s, want = _chains(eg3d_form)
    before = _live()
    for k, v in FORCED:
        monkeypatch.setenv(k, v)
    ctx = api.Context(s.scene)
    ctx.upload_seeds(s.seeds)
    ctx.set_pipelining(3, 5)
    cloud, retried = _traced(capfd, ctx, s.n_seeds)
    assert retried == set(RETRIES)
    _same(cloud, want, CLOUD)
    ctx.set_pipelining(1, 0)
    cloud, retried = _traced(capfd, ctx, s.n_seeds)
    assert retried == set()
    _same(cloud, want, CLOUD)
    ctx.close()
    assert _live() == before


def test_clone_of_a_clone_outlives_both(tiny):
    before = _live()
    parent = api.Context(tiny.scene)
    parent.upload_seeds(tiny.seeds)
    n = tiny.n_seeds
    want = parent.match_resident(0, n)
    assert want["n_points"] > 0
    middle = parent.clone()
    grandchild = middle.clone()
    for c in (middle, grandchild):             # (each now owns work buffers: closing it must give bytes back)
        _same(c.match_resident(0, n), want, CLOUD)
    all_three = _live()
    parent.close()
    two = _live()
    middle.close()
    one = _live()
    assert before < one < two < all_three
    _same(grandchild.match_resident(0, n), want, CLOUD)
    grandchild.close()
    assert _live() == before


def test_seeds_replaced_under_a_clone(tiny):
    """An upload gives the context fresh seeds; a clone made before it keeps matching the ones it was made with."""
    before = _live()
    off, view, xy = tiny.seeds_np()
    n = len(off) - 1
    half = host.SeedsArrays(off[:n // 2 + 1].copy(), view[:off[n // 2]].copy(), xy[:off[n // 2]].copy())
    parent = api.Context(tiny.scene)
    parent.upload_seeds(tiny.seeds)
    want = parent.match_resident(0, n)
    want_half = parent.match_resident(0, n // 2)
    assert 0 < want_half["n_points"] < want["n_points"]
    clone = parent.clone()
    parent.upload_seeds(C.byref(half.c))
    _same(clone.match_resident(0, n), want, CLOUD)
    _same(parent.match_resident(0, n // 2), want_half, CLOUD)
    with pytest.raises(api.Eg3dError) as ei:
        parent.match_resident(0, n // 2 + 1)
    assert "eg3d_match_resident: bad arguments (seeds uploaded?)" in str(ei.value)
    parent.close()
    _same(clone.match_resident(0, n), want, CLOUD)
    clone.close()
    assert _live() == before


def test_the_pair_budget_reaches_a_clone(tiny, monkeypatch):
    """EG3D_SIMGRAPH_PAIR_BUDGET is read when a context is created; a clone cuts the clique expansion as its parent does
    (the budget of test_chunked_clique_expansion_grows_and_keeps). The table slots of the community detection:
    test_gpu_louvain.py::test_determinism_and_clone."""
    before = _live()
    ctx = api.Context(tiny.scene)
    _, want = _every_stage(ctx, tiny)
    ctx.close()
    n_inst, n_edges = want["stats"]["n_pair_instances"], want["stats"]["n_edges"]
    monkeypatch.setenv("EG3D_SIMGRAPH_PAIR_BUDGET", str(max(1, min(n_inst // 3, n_edges // 2))))
    parent = api.Context(tiny.scene)
    monkeypatch.delenv("EG3D_SIMGRAPH_PAIR_BUDGET")
    parent.upload_seeds(tiny.seeds)
    clone = parent.clone()
    got = clone.similarity_graph(None, 0, tiny.n_seeds)
    assert got["stats"]["n_chunks"] >= 3 and want["stats"]["n_chunks"] == 1
    _same(got, want, GRAPH)
    assert got["n_nodes"] == want["n_nodes"]
    clone.close()
    parent.close()
    assert _live() == before
