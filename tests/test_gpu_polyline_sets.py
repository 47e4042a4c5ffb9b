"""-m gpu: the pipelines 1-2 extractor (eg3d_match_polyline_sets: k_n1_samples, k_n1_hits, then the shared consensus and
expand stages) on irregular sets (tests/sets_cases.py) against the oracle, bit for bit: small sets that put dozens of
sets in one wavefront, rows empty in all views but one, long runs of empty rows, overlapping sets, ids of polylines the
walk gives up on, samples and epipolar lines exactly on vertices, and unit cutting on both sides of its bound. Each family
also checks sub-ranges against the slice of the whole call, the pipelined forms of the call against each other, and
enough coverage that the test cannot pass on inputs that miss the branch it was built for."""
import ctypes as C

import numpy as np
import pytest

import sets_cases as cases
from edgegraph3d_amd import api
from parity_util import compare_edgepoints

pytestmark = pytest.mark.gpu

ARRAYS = ("X", "obs_off", "obs_view", "obs_pl", "obs_seg", "obs_xy", "key")
COUNTS = ("n_points", "n_obs", "n_tasks", "n_hypotheses", "n_chains", "flags")


def _oracle(scene_ptr):
    from oracle import binding as ob
    return ob.Oracle(scene_ptr)


@pytest.fixture(scope="module")
def have_gpu():
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"


# (every test names eg3d_form: that is what loads the library of the form and sets the oracle's mode, tests/conftest.py)
@pytest.fixture(scope="module", params=sorted(cases.FAMILIES))
def case(request):
    return cases.FAMILIES[request.param]()


def _parity(ref, got, what):
    rep = compare_edgepoints(ref, got)
    assert rep["ok"] and rep["bitexact_X"] and rep["bitexact_xy"], (what, rep["msgs"][:3])
    assert got["n_tasks"] == ref["n_tasks"] == ref["stats"]["n_tasks"], what
    assert got["n_chains"] == ref["n_chains"], what
    assert got["times"]["bytes_algorithmic"] == ref["stats"]["bytes_algorithmic"], what
    assert got["flags"] & 7 == 0, (what, got["flags"])
    # EG3D_FLAG_DIR_MISMATCH: the oracle counts every Q15 walk (the expand stage's included) the way the kernels do
    assert got["flags"] & 8 == ref["flags"] & 8, (what, got["flags"], ref["flags"])


def _same(a, b, what):
    for k in COUNTS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ARRAYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)


def _slice(whole, s0, s1):
    """the points of `whole` whose sample (key[0]) lies in [s0, s1), keys and offsets rebased"""
    k = whole["key"]
    sel = np.nonzero((k[:, 0] >= s0) & (k[:, 0] < s1))[0]
    p0, p1 = (int(sel[0]), int(sel[-1]) + 1) if len(sel) else (0, 0)
    assert p1 - p0 == len(sel), "the points of a run of samples are contiguous"
    off = whole["obs_off"]
    o0, o1 = int(off[p0]), int(off[p1])
    key = k[p0:p1].copy()
    key[:, 0] -= np.uint32(s0)
    return {"n_points": p1 - p0, "n_obs": o1 - o0, "X": whole["X"][p0:p1], "obs_off": off[p0:p1 + 1] - np.uint64(o0),
            "obs_view": whole["obs_view"][o0:o1], "obs_pl": whole["obs_pl"][o0:o1], "obs_seg": whole["obs_seg"][o0:o1],
            "obs_xy": whole["obs_xy"][o0:o1], "key": key}


def test_irregular_sets_parity(have_gpu, case, eg3d_form):
    n, row_off, ids = case.csr()
    assert cases.rows_strictly_ascending(n, row_off, ids, case.V)
    sa = case.scene_arrays()
    o = _oracle(C.byref(sa.c))
    ctx = api.Context(C.byref(sa.c))
    ctx.set_pipelining(1, 0)
    got = ctx.match_polyline_sets(n, row_off, ids)
    ref = o.match_polyline_sets(n, row_off, ids, nthreads=16)
    _parity(ref, got, case.name)
    counts = o.count_set_samples(n, row_off, ids)
    assert int(counts.sum()) == got["n_tasks"]
    base = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])

    # sub-ranges = the slice of the whole call (and the oracle's sub-range)
    for b, e in case.subranges:
        part = ctx.match_polyline_sets(n, row_off, ids, b, e)
        want = _slice(got, int(base[b]), int(base[e]))
        rep = compare_edgepoints(want, part)
        assert rep["ok"] and rep["bitexact_X"] and rep["bitexact_xy"], (case.name, b, e, rep["msgs"][:3])
        assert part["n_tasks"] == int(base[e] - base[b]), (case.name, b, e)
        assert part["n_chains"] == len(np.unique(want["key"][:, :3], axis=0)), (case.name, b, e)
        _parity(o.match_polyline_sets(n, row_off, ids, b, e, nthreads=16), part, (case.name, b, e))

    # the pipelined forms of the call: byte for byte the same, host arrays and device view
    outs = {}
    for lanes, units in ((1, 0), (3, 0), (3, n)):
        ctx.set_pipelining(lanes, units)
        h = ctx.match_polyline_sets(n, row_off, ids)
        d = ctx.match_polyline_sets(n, row_off, ids, device_only=True)
        dev = ctx.fetch_device_output()
        for k in ("n_points", "n_obs", "n_tasks", "n_chains", "flags"):
            assert d[k] == h[k], (case.name, lanes, units, k)
        outs[(lanes, units)] = (h, dev)
    h0, d0 = outs[(1, 0)]
    _same(got, h0, (case.name, "repeat"))
    for key, (h, dev) in outs.items():
        _same(h0, h, (case.name, "host", key))
        for k in ARRAYS:
            assert np.array_equal(np.ascontiguousarray(dev[k]).view(np.uint8), np.ascontiguousarray(h0[k]).view(np.uint8)), \
                (case.name, "device", key, k)
    _coverage(case, o, ctx, n, row_off, ids, counts, got)
    ctx.close()


def _coverage(case, o, ctx, n, row_off, ids, counts, got):
    """What each family was built to reach, asserted so that the test cannot pass vacuously."""
    spw = cases.sets_per_wave(counts)
    multi = sum(1 for x in spw if x > 1)
    assert multi >= 3, (case.name, "waves that span more than one set", multi)
    assert got["n_points"] > 0, case.name
    if case.name == "tiny":
        assert max(spw) >= 32, ("tiny: the widest wave spans %d sets" % max(spw))
        assert multi >= 10
    elif case.name == "one_view":
        single = sum(1 for s in case.sets if len(s) == 1)
        assert single >= 15, single
    elif case.name == "sparse":
        assert sum(1 for s in case.sets if not s) >= 5
        assert sum(1 for s in case.sets if 0 < len(s) <= 2) >= 10
    elif case.name == "overlap":
        seen = {}
        for s in case.sets:
            for v, ps in s.items():
                for p in ps:
                    seen[(v, p)] = seen.get((v, p), 0) + 1
        assert sum(1 for c in seen.values() if c >= 3) >= 50
    elif case.name == "degenerate":
        walked = {"loop": 0, "invalid": 0, "short": 0, "plain": 0}
        for s in case.sets:
            for v, ps in s.items():
                for p in ps:
                    walked[case.kind(v, p)] += 1
        assert walked["loop"] >= 10 and walked["invalid"] >= 10 and walked["short"] >= 10, walked
        # valid polylines of exactly 2 vertices that hold samples (k_n1_samples walks polylines of pl.n >= 2)
        two = [(v, p) for s in case.sets for v, ps in s.items() for p in ps
               if case.kind(v, p) == "plain" and len(case.polyline(v, p)) == 2]
        assert sum(len(o.polyline_samples(v, p)[0]) for v, p in two) >= 50, len(two)
        # the last three sets hold only loops / invalid / short polylines. The extractor walks towards pl.end; for a loop
        # pl.end == pl.start and next_pl_point_by_distance tests `direction == start` first (polyline_graph_2d.cpp:398):
        # the walk goes towards the start it stands on and reaches it at once — no sample, and no Q15 report (bit 8), since
        # the direction IS an end of the polyline. Invalid polylines and those of < 2 vertices are never walked; a
        # valid segment under 20 px reaches its end before any sample.
        for i in range(n - 3, n):
            r = ctx.match_polyline_sets(n, row_off, ids, i, i + 1)
            assert r["n_tasks"] == 0 and r["n_points"] == 0 and r["flags"] == 0, (i, r["n_tasks"], r["flags"])
    elif case.name == "exact":
        on_vertex = 0
        for v in range(case.V):
            for p in range(case.n_pl(v)):
                xy, _ = o.polyline_samples(v, p)
                vt = case.polyline(v, p)
                on_vertex += int((xy[:, None, :] == vt[None, :, :]).all(axis=2).any(axis=1).sum())
        assert on_vertex >= 100, on_vertex
        # epipolar lines y = const through a vertex shared by two segments: both report t in [0, 1] (Q10); the chains
        # hold observations exactly on vertices in views other than the start view
        obs_on_vertex = 0
        for v in range(case.V):
            m = got["obs_view"] == v
            pts = got["obs_xy"][m]
            pls = got["obs_pl"][m]
            for p in np.unique(pls):
                vt = case.polyline(v, int(p))
                q = pts[pls == p]
                obs_on_vertex += int((q[:, None, :] == vt[None, :, :]).all(axis=2).any(axis=1).sum())
        assert obs_on_vertex >= 100, obs_on_vertex
    elif case.name.startswith("bound"):
        mx = case.meta["max_items"]
        sizes = [int(row_off[(i + 1) * case.V] - row_off[i * case.V]) for i in range(n)]
        assert sizes[0] + sizes[1] == mx and sizes[2] + sizes[3] == mx + 1 and sizes[4] > mx, sizes
        ctx.set_pipelining(1, 0)
        for b, e, units in case.units:
            assert cases.units_expected(row_off, case.V, b, e, mx) == units
            r = ctx.match_polyline_sets(n, row_off, ids, b, e)
            assert r["n_points"] > 0
            # every set of these ranges emits chains and fits one expand launch, so the call's pieces = its units, and the
            # device view of a host call is complete exactly when the range ran as one unit (include/eg3d.h)
            assert ctx.last_device_output().complete == (1 if units == 1 else 0), (case.name, b, e, units)
        n_units = sum(u for _, _, u in case.units)
        assert n_units == 10, n_units


def test_rows_must_be_strictly_ascending(have_gpu, eg3d_form):
    """include/eg3d.h: ids are strictly ascending within a row (the reference's set<ulong>). A repeated id would be
    sampled and scanned twice; an unsorted row reorders the output. Both are refused with EG3D_ERR_ARG, and the context
    stays usable."""
    c = cases.overlap()
    n, row_off, ids = c.csr()
    sa = c.scene_arrays()
    ctx = api.Context(C.byref(sa.c))
    good = ctx.match_polyline_sets(n, row_off, ids, 0, 3)
    r = next(r for r in range(n * c.V) if row_off[r + 1] - row_off[r] >= 3)
    a = int(row_off[r])
    dup = ids.copy()
    dup[a + 1] = dup[a]
    swapped = ids.copy()
    swapped[a], swapped[a + 1] = ids[a + 1], ids[a]
    for bad, what in ((dup, "duplicate"), (swapped, "unsorted")):
        ne = api.lib().eg3d_last_error
        with pytest.raises(api.Eg3dError) as ei:
            ctx.match_polyline_sets(n, row_off, bad)
        assert "rc=-1" in str(ei.value), what
        assert b"not strictly ascending" in ne(), what
        # the check covers every row of the sets, not only those of the range
        with pytest.raises(api.Eg3dError):
            ctx.match_polyline_sets(n, row_off, bad, n - 1, n)
        _same(good, ctx.match_polyline_sets(n, row_off, ids, 0, 3), what)
    ctx.close()


def test_null_pl_ids_is_refused_before_an_id_is_read(have_gpu, eg3d_form):
    """A CSR whose row_off names ids while the pl_ids pointer is null is refused by the argument checks of both entry
    points on host sets — EG3D_ERR_ARG, "pl_ids is null", no id read, no kernel launched — and the context stays usable."""
    from edgegraph3d_amd import _cdefs as D
    c = cases.overlap()
    n, row_off, ids = c.csr()
    assert row_off[-1] > 0
    sa = c.scene_arrays()
    ctx = api.Context(C.byref(sa.c))
    good = ctx.match_polyline_sets(n, row_off, ids, 0, 3)
    L = api.lib()
    ps = D.PolylineSets(n, D.np_ptr(row_off, C.c_uint32), None)
    e, tm, sc = D.EdgePoints(), D.StageTimes(), D.SetCandidates()
    assert L.eg3d_match_polyline_sets(ctx._h, C.byref(ps), 0, n, 0, C.byref(e), C.byref(tm)) == -1  # EG3D_ERR_ARG
    assert b"pl_ids is null" in L.eg3d_last_error()
    assert L.eg3d_polyline_set_candidates(ctx._h, C.byref(ps), 0, n, None, C.byref(sc)) == -1
    assert b"pl_ids is null" in L.eg3d_last_error()
    _same(good, ctx.match_polyline_sets(n, row_off, ids, 0, 3), "after the refusals")
    ctx.close()
