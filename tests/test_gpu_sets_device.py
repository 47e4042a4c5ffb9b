"""-m gpu: include/eg3d_sets_device.h — polyline sets that stay on the device and the extractor cut by polyline.

  K13       eg3d_sets_from_communities_device against the host statement (host.sets_from_communities) and the Python one
            (tests/simgraph_ref.py), as row_off / pl_ids bytes: K11's ids read on the device, and caller ids.
  upload    eg3d_upload_polyline_sets gives the bytes back and refuses, by its device check, what eg3d_match_polyline_sets
            refuses on the host, with the same texts.
  items     eg3d_match_polyline_items over the whole range equals eg3d_match_polyline_sets byte for byte; cut inside a set
            (after its first item, in the middle of a row, at a row boundary) the pieces concatenate to the same bytes;
            eg3d_polyline_item_samples equals the oracle's walk; a small EG3D_ITEM_UNIT_SAMPLES cuts one set into several
            units with the same bytes on 1 and 3 lanes, host arrays and device view; matched intervals on the device;
            EG3D_TEST_ITEM_WRAP makes a unit count as one whose 32-bit totals wrap: cut in two, redone, same bytes.
  chains    pipeline 1 (graph -> communities -> K13 -> items) and pipeline 2 (K9 -> items) without the host rows.

Not reachable through this interface, so not tested here: a node whose view is >= V (K13 reads node_view where
eg3d_similarity_graph left it; no call uploads a graph's nodes), and a (view, polyline) named twice in one community (the
nodes of that graph are distinct polylines). The kernel's checks for both are stated in csrc/eg3d_k13_sets.hip."""
import ctypes as C
import os

import numpy as np
import pytest

import sets_cases as cases
import simgraph_ref as sref
from edgegraph3d_amd import api, host
from parity_util import compare_edgepoints

pytestmark = pytest.mark.gpu

ARRAYS = ("X", "obs_off", "obs_view", "obs_pl", "obs_seg", "obs_xy", "key")
COUNTS = ("n_points", "n_obs", "n_tasks", "n_hypotheses", "n_chains", "flags")
_CASES = {}   # name -> Case (form-independent: scenes and sets only), built once and never modified
_SYNTH = {}


def _synth(cfg):
    if cfg not in _SYNTH:
        _SYNTH[cfg] = host.Synth(cfg)
    return _SYNTH[cfg]


def merged():
    """Synth(1)'s curve sets merged into two sets (even curves, odd curves): every row holds many polylines."""
    s = _synth(1)
    sc, cur = cases._curves(s)
    V = int(sc["n_views"])
    sets = [{v: sorted(p for c in range(k, len(cur), 2) for p in cur[c][v]) for v in range(V)} for k in (0, 1)]
    sets = [{v: ps for v, ps in st.items() if ps} for st in sets]
    return cases.Case("merged", sc, sets)


FAMILIES = {"tiny": cases.tiny, "sparse": cases.sparse, "merged": merged}


def _case(name):
    if name not in _CASES:
        _CASES[name] = FAMILIES[name]()
    return _CASES[name]


def _context(scene_ptr, **env):
    """A fresh context; the EG3D_* knobs are read when a context is created."""
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    old = {k: os.environ.pop(k, None) for k in env}
    try:
        os.environ.update({k: str(v) for k, v in env.items()})
        return api.Context(scene_ptr)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _live():
    f = api.lib().eg3d_test_live_device_bytes
    f.restype, f.argtypes = C.c_int64, []
    return int(f())


def _same(a, b, what):
    for k in COUNTS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ARRAYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)


def _concat(parts):
    """The clouds of adjacent item ranges as one: arrays appended, observation offsets rebased, counts summed."""
    out = {k: sum(p[k] for p in parts) for k in COUNTS if k != "flags"}
    out["flags"] = int(np.bitwise_or.reduce([p["flags"] for p in parts]))
    for k in ARRAYS:
        if k != "obs_off":
            out[k] = np.concatenate([p[k] for p in parts])
    off, base = [], 0
    for p in parts:
        off.append(p["obs_off"][:-1] + np.uint64(base))
        base += int(p["n_obs"])
    out["obs_off"] = np.concatenate(off + [np.array([base], np.uint64)])
    return out


def _same_sets(got, want, what):
    assert got[0] == want[0], (what, got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        g, w = np.ascontiguousarray(g, np.uint32), np.ascontiguousarray(w, np.uint32)
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), what


# ---- K13 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,n_seeds", [(0, None), (2, 2000)], ids=["config0", "config2_first_2000"])
def test_k13_equals_the_host_statement(cfg, n_seeds, eg3d_form):
    s = _synth(cfg)
    n_seeds = s.n_seeds if n_seeds is None else n_seeds
    ctx = _context(s.scene)
    V = ctx.n_views
    g = ctx.similarity_graph(s.seeds, 0, n_seeds)
    n = int(g["n_nodes"])
    assert n >= 20
    com = ctx.communities(g)
    # K11's ids, read where eg3d_detect_communities left them
    view, st = ctx.sets_from_communities_device(None, n=n, with_stats=True)
    want = host.sets_from_communities(g, com["ids"], V)
    _same_sets(ctx.fetch_polyline_sets(view), want, "K11's ids")
    _same_sets(sref.sets_from_communities(g, com["ids"], V), want, "the Python statement")
    assert (view.n_sets, view.n_views, view.device, view.n_ids) == (want[0], V, ctx.device, len(want[2]))
    assert (st["n_nodes"], st["n_named"], st["n_sets"], st["n_ids"]) == (n, int((com["ids"] >= 0).sum()), want[0], len(want[2]))
    print("K13 config %d: %d nodes, %d sets, %d ids, %.3f ms on the device" % (cfg, n, want[0], len(want[2]), st["ms_device"]))
    # the caller's ids
    rng = np.random.default_rng(5 + cfg)
    holes = com["ids"].copy() * 3 + 2                      # gaps: communities 0, 1, 3, 4, 6, ... are named by nobody
    holes[rng.random(n) < 0.3] = -1                        # ... and nodes that belong to none
    holes[0] = -7
    relabel = rng.permutation(int(com["ids"].max()) + 1).astype(np.int64)
    shuffled = np.where(com["ids"] >= 0, relabel[np.maximum(com["ids"], 0)], -1)
    variants = {"holes": holes, "one id for all": np.full(n, 4, np.int64), "every node its own": rng.permutation(n).astype(np.int64),
                "shuffled": shuffled, "nobody named": np.full(n, -1, np.int64)}
    for what, ids in variants.items():
        want = host.sets_from_communities(g, ids, V)
        _same_sets(ctx.fetch_polyline_sets(ctx.sets_from_communities_device(ids)), want, what)
        _same_sets(sref.sets_from_communities(g, ids, V), want, (what, "the Python statement"))
    assert host.sets_from_communities(g, holes, V)[0] == int(holes.max()) + 1
    # the result feeds the extractor as it is
    v2 = ctx.sets_from_communities_device(shuffled)
    counts = ctx.polyline_item_samples(v2)
    assert len(counts) == v2.n_ids and counts.sum() > 0
    ctx.close()


def test_k13_refusals(eg3d_form):
    s = _synth(0)
    ctx = _context(s.scene)
    err = api.lib().eg3d_last_error
    with pytest.raises(api.Eg3dError) as ei:                       # no graph on this context yet
        ctx.sets_from_communities_device(np.zeros(3, np.int64))
    assert "rc=-1" in str(ei.value) and b"no eg3d_similarity_graph call" in err()
    g = ctx.similarity_graph(s.seeds)
    n = int(g["n_nodes"])
    for bad_n in (n - 1, n + 1, 0):
        with pytest.raises(api.Eg3dError) as ei:                   # wrong n
            ctx.sets_from_communities_device(np.zeros(bad_n, np.int64))
        assert "rc=-1" in str(ei.value) and b"n is not the n_nodes" in err()
    with pytest.raises(api.Eg3dError) as ei:                       # NULL ids before any community call
        ctx.sets_from_communities_device(None, n=n)
    assert b"no eg3d_detect_communities call" in err()
    big = np.zeros(n, np.int64)
    big[1] = (1 << 32) // ctx.n_views + 1                          # sets x views reaches 2^32 - 1
    with pytest.raises(api.Eg3dError) as ei:
        ctx.sets_from_communities_device(big)
    assert "rc=-3" in str(ei.value), str(ei.value)
    with pytest.raises(RuntimeError):
        host.sets_from_communities(g, big, ctx.n_views)            # (the host statement refuses it too)
    # the context stays usable, and a refused call leaves no current view behind
    ids = np.arange(n, dtype=np.int64) % 5
    v = ctx.sets_from_communities_device(ids)
    _same_sets(ctx.fetch_polyline_sets(v), host.sets_from_communities(g, ids, ctx.n_views), "after the refusals")
    with pytest.raises(api.Eg3dError):
        ctx.sets_from_communities_device(big)
    with pytest.raises(api.Eg3dError):
        ctx.polyline_item_samples(v)
    assert b"not a current device view" in err()
    ctx.close()


# ---- upload ---------------------------------------------------------------------------------------------------------------
def test_upload_gives_the_bytes_back_and_refuses_on_the_device(eg3d_form):
    c = cases.overlap()
    n, row_off, ids = c.csr()
    sa = c.scene_arrays()
    ctx = _context(C.byref(sa.c))
    err = api.lib().eg3d_last_error
    good = ctx.upload_polyline_sets(n, row_off, ids)
    _same_sets(ctx.fetch_polyline_sets(good), (n, row_off, ids), "upload")
    want = ctx.match_polyline_sets(n, row_off, ids, 0, 3)
    i3 = int(row_off[3 * c.V])
    _same(want, ctx.match_polyline_items(good, 0, i3), "sets [0, 3) as items")
    # the rows of test_rows_must_be_strictly_ascending (tests/test_gpu_polyline_sets.py)
    r = next(r for r in range(n * c.V) if row_off[r + 1] - row_off[r] >= 3)
    a = int(row_off[r])
    dup = ids.copy()
    dup[a + 1] = dup[a]
    swapped = ids.copy()
    swapped[a], swapped[a + 1] = ids[a + 1], ids[a]
    at_count = ids.copy()
    at_count[a + 2] = c.n_pl(r % c.V)            # an id equal to its view's polyline count (the row stays ascending)
    assert at_count[a + 2] > at_count[a + 1]
    r2 = next(q for q in range(n * c.V) if row_off[q] > 0 and row_off[q + 1] > row_off[q])
    descending = row_off.copy()
    descending[r2 + 1] = descending[r2] - 1      # row r2 ends before it begins
    for bad_off, bad_ids, text in ((row_off, dup, b"not strictly ascending"), (row_off, swapped, b"not strictly ascending"),
                                   (row_off, at_count, b"polyline id out of range"), (descending, ids, b"row_off is not ascending")):
        with pytest.raises(api.Eg3dError) as ei:
            ctx.upload_polyline_sets(n, bad_off, bad_ids)
        assert "rc=-1" in str(ei.value), text
        assert text in err(), (text, err())
        with pytest.raises(api.Eg3dError):       # the host call refuses the same sets ...
            ctx.match_polyline_sets(n, bad_off, bad_ids)
        assert text in err(), (text, err())      # ... with the same text
        with pytest.raises(api.Eg3dError):       # a refused upload ends the view before it
            ctx.match_polyline_items(good, 0, i3)
        good = ctx.upload_polyline_sets(n, row_off, ids)   # the context stays usable
        _same(want, ctx.match_polyline_items(good, 0, i3), text)
    # the host call uploads into buffers of its own: the view outlives it
    ctx.match_polyline_sets(n, row_off, ids, 0, 2)
    _same(want, ctx.match_polyline_items(good, 0, i3), "after a host call")
    ctx.close()


# ---- the extractor on item ranges ------------------------------------------------------------------------------------------
def _cuts_inside_a_set(row_off, V, n_sets):
    """item indices strictly inside a set: after its first item; in the middle of a row; at a row boundary"""
    firsts, mids, rows = [], [], []
    for s in range(n_sets):
        b, e = int(row_off[s * V]), int(row_off[(s + 1) * V])
        if e - b >= 2:
            firsts.append(b + 1)
        for v in range(V):
            rb, re = int(row_off[s * V + v]), int(row_off[s * V + v + 1])
            if re - rb >= 2:
                mids.append(rb + (re - rb) // 2)
            if b < re < e and re > rb:
                rows.append(re)
    # spread over the range, so that the pieces between them hold points: an early set, a middle one, a late one
    first = firsts[len(firsts) // 3] if firsts else None
    mids = [m for m in mids if m != first]
    mid = mids[len(mids) // 2] if mids else None
    rows = [r for r in rows if r not in (first, mid)]
    row = rows[-1 - len(rows) // 4] if rows else None
    return first, mid, row


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_items_equal_the_sets_call_whole_and_cut(name, eg3d_form):
    from oracle import binding as ob
    case = _case(name)
    n, row_off, ids = case.csr()
    V = case.V
    sa = case.scene_arrays()
    ctx = _context(C.byref(sa.c))
    ctx.set_pipelining(1, 0)
    whole = ctx.match_polyline_sets(n, row_off, ids)
    assert whole["n_points"] > 0
    view = ctx.upload_polyline_sets(n, row_off, ids)
    n_items = int(view.n_ids)
    assert n_items == len(ids)
    got = ctx.match_polyline_items(view)
    _same(whole, got, (name, "whole range"))
    # per-item counts = the oracle's walk of each polyline
    counts = ctx.polyline_item_samples(view)
    o = ob.Oracle(C.byref(sa.c))
    memo = {}
    for r in range(n * V):
        for k in range(int(row_off[r]), int(row_off[r + 1])):
            key = (r % V, int(ids[k]))
            if key not in memo:
                memo[key] = len(o.polyline_samples(*key)[0])
            assert counts[k] == memo[key], (name, k, key)
    o.close()
    assert int(counts.sum()) == whole["n_tasks"]
    prefix = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    sub = ctx.polyline_item_samples(view, 3, min(n_items, 40))
    assert np.array_equal(sub, counts[3:min(n_items, 40)])
    # cut inside a set: the pieces, each given the samples before it, concatenate to the same bytes
    first, mid, row = _cuts_inside_a_set(row_off, V, n)
    assert first is not None and row is not None, name
    if name == "merged":
        assert mid is not None
    cuts = sorted({c for c in (first, mid, row) if c is not None})
    bounds = [0] + cuts + [n_items]
    parts = [ctx.match_polyline_items(view, b, e, sample_base=int(prefix[b])) for b, e in zip(bounds[:-1], bounds[1:])]
    for p, b, e in zip(parts, bounds[:-1], bounds[1:]):
        assert p["n_tasks"] == int(prefix[e] - prefix[b]), (name, b, e)
    _same(whole, _concat(parts), (name, "cut at", cuts))
    assert sum(1 for p in parts if p["n_points"]) >= 2, name
    # an empty range, and a range outside the sets
    empty = ctx.match_polyline_items(view, first, first, sample_base=5)
    assert empty["n_points"] == 0 and empty["n_tasks"] == 0 and empty["n_units"] == 0
    with pytest.raises(api.Eg3dError):
        ctx.match_polyline_items(view, 0, n_items + 1)
    ctx.close()


def test_a_set_larger_than_a_unit_is_cut_inside(eg3d_form):
    case = _case("merged")
    n, row_off, ids = case.csr()
    sa = case.scene_arrays()
    ctx0 = _context(C.byref(sa.c))
    ctx0.set_pipelining(1, 0)
    want = ctx0.match_polyline_sets(n, row_off, ids)
    counts = ctx0.polyline_item_samples(ctx0.upload_polyline_sets(n, row_off, ids))
    ctx0.close()
    per_set = [int(counts[int(row_off[s * case.V]):int(row_off[(s + 1) * case.V])].sum()) for s in range(n)]
    cap = max(int(counts.max()), min(per_set) // 5)       # every set is at least 5 units' worth; no single polyline above a unit
    assert n == 2 and min(per_set) >= 5 * cap

    def greedy(b, e):   # the cut of one lane: item ranges of at most `cap` samples, at least one item each
        units, i0 = 0, b
        while i0 < e:
            i1, acc = i0 + 1, int(counts[i0])
            while i1 < e and acc + int(counts[i1]) <= cap:
                acc += int(counts[i1])
                i1 += 1
            units += 1
            i0 = i1
        return units

    ctx = _context(C.byref(sa.c), EG3D_ITEM_UNIT_SAMPLES=cap)
    view = ctx.upload_polyline_sets(n, row_off, ids)
    for lanes in (1, 3):
        ctx.set_pipelining(lanes, 0)
        h = ctx.match_polyline_items(view)
        assert h["n_units"] >= 2 * 4, (lanes, h["n_units"])     # each of the two sets became at least 4 units
        if lanes == 1:
            assert h["n_units"] == greedy(0, len(ids))
        _same(want, h, ("host arrays", lanes))
        d = ctx.match_polyline_items(view, device_only=True)
        assert d["n_units"] == h["n_units"]
        dev = ctx.fetch_device_output()
        for k in ARRAYS:
            assert np.array_equal(np.ascontiguousarray(dev[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), \
                ("device view", lanes, k)
    ctx.close()


def test_a_unit_whose_totals_wrap_is_cut_in_two_and_redone(eg3d_form):
    """EG3D_TEST_ITEM_WRAP below the hit total of the smaller merged set: whatever unit holds a whole set counts as one
    whose 32-bit totals wrap, is cut in two by its samples and redone — the bytes stay those of the uncut call."""
    case = _case("merged")
    n, row_off, ids = case.csr()
    sa = case.scene_arrays()
    ctx0 = _context(C.byref(sa.c))
    ctx0.set_pipelining(1, 0)
    want = ctx0.match_polyline_sets(n, row_off, ids)
    hits = [int(ctx0.polyline_set_candidates(n, row_off, ids, s, s + 1)["list_off"][-1]) for s in range(n)]
    plain = ctx0.match_polyline_items(ctx0.upload_polyline_sets(n, row_off, ids))
    assert plain["n_units"] == 1 and plain["n_redone"] == 0
    ctx0.close()
    knob = min(hits) - 1
    assert knob > 1000, hits
    print("merged: %d samples, %d hypotheses, hits per set %s" % (plain["n_tasks"], plain["n_hypotheses"], hits))
    # one lane: the whole range is one unit above the knob. Three lanes: three units of a third of the samples each, so a
    # third of the knob puts each of them above it, and the parts of different units are redone side by side
    for lanes, knob_l in ((1, knob), (3, knob // 3)):
        ctx = _context(C.byref(sa.c), EG3D_TEST_ITEM_WRAP=knob_l)
        view = ctx.upload_polyline_sets(n, row_off, ids)
        ctx.set_pipelining(lanes, 0)
        h = ctx.match_polyline_items(view)
        print("wrap knob %d: %d units, %d redone on %d lane(s)" % (knob_l, h["n_units"], h["n_redone"], lanes))
        assert h["n_redone"] > 0, (lanes, h["n_units"])
        _same(want, h, ("redone, host arrays", lanes))
        d = ctx.match_polyline_items(view, device_only=True)
        assert d["n_redone"] > 0
        dev = ctx.fetch_device_output()
        for k in ARRAYS:
            assert np.array_equal(np.ascontiguousarray(dev[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), \
                ("redone, device view", lanes, k)
        ctx.close()
    # a single polyline above the knob cannot be cut: EG3D_ERR_CAPACITY
    ctx = _context(C.byref(sa.c), EG3D_TEST_ITEM_WRAP=1)
    view = ctx.upload_polyline_sets(n, row_off, ids)
    with pytest.raises(api.Eg3dError) as ei:
        ctx.match_polyline_items(view)
    assert "rc=-3" in str(ei.value) and b"single polyline" in api.lib().eg3d_last_error()
    assert ctx.match_polyline_items(view, 0, 0)["n_points"] == 0      # the context stays usable
    ctx.close()


def test_items_under_matched_intervals_on_the_device(eg3d_form):
    """m = the intervals eg3d_replay_device left on the device after pipeline 3's cloud of Synth(1)."""
    s = _synth(1)
    case = _case("merged")
    n, row_off, ids = case.csr()
    ctx = _context(s.scene)
    ctx.set_pipelining(1, 0)
    ctx.match_refpoints(s.seeds, device_only=True)
    _, dv, st = ctx.replay_device(to_host=False)
    assert int(st["n_intervals"]) > 0
    want = ctx.match_polyline_sets(n, row_off, ids, matched=dv)
    plain = ctx.match_polyline_sets(n, row_off, ids)
    assert want["n_tasks"] < plain["n_tasks"]              # the manager holds something of these sets
    view = ctx.upload_polyline_sets(n, row_off, ids)
    _same(want, ctx.match_polyline_items(view, matched=dv), "matched, whole range")
    counts = ctx.polyline_item_samples(view, matched=dv)
    assert int(counts.sum()) == want["n_tasks"] and int(ctx.polyline_item_samples(view).sum()) == plain["n_tasks"]
    cut = int(row_off[3]) + 1                               # inside a row of the first set
    prefix = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    parts = [ctx.match_polyline_items(view, 0, cut, matched=dv),
             ctx.match_polyline_items(view, cut, len(ids), sample_base=int(prefix[cut]), matched=dv)]
    _same(want, _concat(parts), "matched, cut")
    ctx.close()


# ---- the chains without the host rows --------------------------------------------------------------------------------------
def test_pipeline_1_end_to_end_without_the_host_rows(eg3d_form):
    """Config 0: similarity_graph -> communities -> K13 -> match_polyline_items equals the chain through the host rows
    (test_end_to_end_without_a_file of tests/test_gpu_louvain.py) and the oracle's extractor."""
    from oracle import binding as ob
    s = _synth(0)
    before = _live()
    ctx = _context(s.scene)
    V = ctx.n_views
    g = ctx.similarity_graph(s.seeds)
    com = ctx.communities(g)
    n_sets, row_off, pl_ids = host.sets_from_communities(g, com["ids"], V)
    through_host = ctx.match_polyline_sets(n_sets, row_off, pl_ids)
    view = ctx.sets_from_communities_device(None, n=int(g["n_nodes"]))
    cloud = ctx.match_polyline_items(view)
    _same(through_host, cloud, "pipeline 1")
    assert cloud["n_points"] > 0
    orc = ob.Oracle(s.scene)
    rep = compare_edgepoints(orc.match_polyline_sets(n_sets, row_off, pl_ids), cloud)
    orc.close()
    assert rep["ok"], rep["msgs"]
    # memory: everything the context allocated, lanes and resident sets included, goes with it
    ctx.set_pipelining(3, 6)
    _same(through_host, ctx.match_polyline_items(view), "pipeline 1, 3 lanes")
    assert _live() > before
    ctx.close()
    assert _live() == before


def test_pipeline_2_from_the_rows_k9_left(eg3d_form):
    s = _synth(0)
    ctx = _context(s.scene)
    err = api.lib().eg3d_last_error
    with pytest.raises(api.Eg3dError):
        ctx.polyline_matches_device()
    assert b"no eg3d_match_polylines_closeness call" in err()
    m = ctx.match_polylines_closeness(s.seeds)
    assert m["n_sets"] >= 3
    view = ctx.polyline_matches_device()
    _same_sets(ctx.fetch_polyline_sets(view), (m["n_sets"], m["row_off"], m["pl_ids"]), "K9's rows")
    want = ctx.match_polyline_sets(m["n_sets"], m["row_off"], m["pl_ids"])
    assert want["n_points"] > 0
    _same(want, ctx.match_polyline_items(view), "pipeline 2")
    # the next matcher call ends the view; an empty result is a view of no sets
    ctx.upload_seeds(s.seeds)
    ctx.match_polylines_closeness(None, 7, 7)
    with pytest.raises(api.Eg3dError):
        ctx.match_polyline_items(view)
    none = ctx.polyline_matches_device()
    assert (none.n_sets, none.n_ids) == (0, 0) and list(ctx.fetch_polyline_sets(none)[1]) == [0]
    assert ctx.match_polyline_items(none)["n_points"] == 0
    ctx.close()


def test_example_resident_sets_writes_the_same_file(tmp_path, eg3d_form):
    """examples/edge_matcher_refpoints.cpp on --make-synthetic scene 2: --louvain --match2 with --resident-sets (K13 and
    K9's rows feed the extractor on the device) writes, byte for byte, the file of the run through the host rows."""
    import subprocess

    import cbuild
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path, lib=cbuild.DEFAULT_LIB)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "2", d])
    common = [exe, os.path.join(d, "input.json"), os.path.join(d, "plgs.bin")]
    env = dict(os.environ, EG3D_LIB="")   # (the example links the default library)
    subprocess.check_call(common + [os.path.join(d, "a.json"), "--louvain", "--match2"], env=env)
    out = subprocess.run(common + [os.path.join(d, "b.json"), "--louvain", "--match2", "--resident-sets"], env=env, check=True,
                         capture_output=True, text=True).stdout
    assert "pipeline 1:" in out and "pipeline 2:" in out, out
    a, b = open(os.path.join(d, "a.json"), "rb").read(), open(os.path.join(d, "b.json"), "rb").read()
    assert len(a) > 1000 and a == b
    plain = os.path.join(d, "c.json")
    subprocess.check_call(common + [plain], env=env)
    assert open(plain, "rb").read() != a      # (pipelines 1 and 2 did add points)
