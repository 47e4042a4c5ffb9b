"""-m gpu: K18, the cloud-to-cloud nearest distances on the device (include/eg3d/nearest.hpp) against the sequential statement
eg3d_host_cloud_nearest, bit for bit — all d2, all nn, every figure —, once per product library:
  * every case of tests/nearest_cases.py through nearest_points (host arrays) and nearest_device (arrays uploaded with
    Context.upload), with each lane mapping of the query kernel, and the index's figures;
  * the resident cloud of host.Synth(1) against itself, and after a translation by half of max_dist;
  * compare_clouds against host.compare_clouds, both directions;
  * the device outputs feeding compact_device;
  * the refusals, with canary-filled outputs; empty inputs; the two orders of freeing an index and closing its context.
No test provokes a fault: every refusal is decided on the host, the extent after the reduction that finds it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import nearest_cases as nc
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host

pytestmark = pytest.mark.gpu
F = np.float32
_CTX = {}      # form -> (synth, context) on host.Synth(1)
_WANT = {}     # case name -> the host statement's (d2, nn, figures), computed once
_CLOUD = {}    # form -> the fetched X of the resident cloud


def _ctx(form):
    if form not in _CTX:
        assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
        s = host.Synth(1)
        _CTX[form] = (s, api.Context(s.scene))
    return _CTX[form][1]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    import forms
    for rows in list(_CTX):
        with forms.product_form(rows):   # eg3d_destroy of the library that created the context
            _CTX[rows][1].close()
    _CTX.clear()
    _CLOUD.clear()


def _want(case):
    if case["name"] not in _WANT:
        _WANT[case["name"]] = host.cloud_nearest(case["ref"], case["X"], case["max_dist"], cell=case["cell"], ref_keep=case["ref_keep"],
                                                 keep=case["keep"], thresholds=case["thresholds"])
    return _WANT[case["name"]]


def _resident(form):
    """the context with the cloud of Synth(1) as its last device output, and that cloud's X on the host"""
    ctx = _ctx(form)
    ctx.match_refpoints(_CTX[form][0].seeds, device_only=True)
    if form not in _CLOUD:
        _CLOUD[form] = ctx.fetch_device_output()["X"].copy()
    return ctx, _CLOUD[form]


@pytest.mark.parametrize("group", ("default", "1", "8", "64"))
@pytest.mark.parametrize("case", nc.CASES, ids=nc.IDS)
def test_case_against_the_host_statement(eg3d_form, case, group, monkeypatch):
    if group == "default":
        monkeypatch.delenv("EG3D_K18_GROUP", raising=False)
    else:
        monkeypatch.setenv("EG3D_K18_GROUP", group)     # (read when the index is built)
    ctx, want = _ctx(eg3d_form), _want(case)
    with ctx.cloud_index(X=case["ref"], keep=case["ref_keep"], cell=case["cell"]) as index:
        hs = host.cloud_index_stats(case["ref"], case["cell"], case["ref_keep"])
        for f in ("n_points", "n_dropped", "n_nonfinite", "n_indexed", "n_cells", "max_cell_points", "dims"):
            assert index.stats[f] == hs[f], (f, index.stats[f], hs[f])
        assert np.array_equal(index.stats["origin"], hs["origin"]) and index.n_indexed == hs["n_indexed"] and index.n_cells == hs["n_cells"]
        got = ctx.nearest_points(index, case["X"], case["max_dist"], keep=case["keep"], thresholds=case["thresholds"])
        nc.assert_same(got, want, case["name"] + " nearest_points")
        if group in ("default", "8"):
            n = len(case["X"])
            Xd = ctx.upload(case["X"] if n else np.zeros(3, F))
            kd = None if case["keep"] is None else ctx.upload(case["keep"] if n else np.zeros(1, np.uint8))
            r = ctx.nearest_device(index, case["max_dist"], cloud=api.points_cloud(Xd, n), keep=kd.ptr if kd is not None else None,
                                   thresholds=case["thresholds"])
            nc.assert_same((r["d2"][:n], r["nn"][:n], r["stats"]), want, case["name"] + " nearest_device")
    # the same reference indexed from the device
    if group == "default" and len(case["ref"]):
        Rd = ctx.upload(case["ref"])
        rk = None if case["ref_keep"] is None else ctx.upload(case["ref_keep"])
        with ctx.cloud_index(cloud=api.points_cloud(Rd, len(case["ref"])), keep=rk, cell=case["cell"]) as index:
            assert index.stats["n_cells"] == hs["n_cells"] and index.stats["max_cell_points"] == hs["max_cell_points"]
            nc.assert_same(ctx.nearest_points(index, case["X"], case["max_dist"], keep=case["keep"], thresholds=case["thresholds"]), want,
                           case["name"] + " index_build_device")


def test_resident_cloud_against_itself_and_after_a_translation(eg3d_form):
    ctx, X = _resident(eg3d_form)
    n = len(X)
    finite = np.isfinite(X).all(axis=1)
    assert n > 1000 and finite.sum() > 1000
    extent = float(np.ptp(X[finite], axis=0).max())
    md = float(F(0.01 * extent))
    with ctx.cloud_index(cell=md) as index:          # the last device output, built BEFORE the transform
        assert index.stats["n_points"] == n and index.n_indexed == int(finite.sum())
        r = ctx.nearest_device(index, md, thresholds=(md,))
        d2, nn, st = r["d2"], r["nn"], r["stats"]
        assert (d2[finite] == 0).all() and np.isinf(d2[~finite]).all()
        assert (nn[finite] <= np.nonzero(finite)[0]).all()
        first = {}
        for i in np.nonzero(finite)[0]:
            first.setdefault(tuple((X[i] + F(0)).tolist()), int(i))     # (-0 and +0 are the same coordinate)
        assert [int(v) for v in nn[finite]] == [first[tuple((X[i] + F(0)).tolist())] for i in np.nonzero(finite)[0]]
        assert st["n_within"] == int(finite.sum()) and st["sum_q32"] == 0 and st["n_below"] == [int(finite.sum())]
        nc.assert_same((d2, nn, st), host.cloud_nearest(X, X, md, thresholds=(md,)), "self")
        T = np.eye(4)
        T[0, 3] = 0.5 * md
        ctx.transform_device(T)
        moved = ctx.fetch_device_output()["X"]
        r = ctx.nearest_device(index, md, thresholds=(md, 0.75 * md))
        want = host.cloud_nearest(X, moved, md, thresholds=(md, 0.75 * md))
        nc.assert_same((r["d2"], r["nn"], r["stats"]), want, "translated")
        if finite.all():
            assert r["stats"]["n_within"] == n
        assert r["stats"]["n_within"] == int(np.isfinite(moved).all(axis=1).sum())
        print("Synth(1): %d points, %d cells (largest %d), lanes per query by default; build %.3f ms, query %.3f ms" %
              (n, index.n_cells, index.stats["max_cell_points"], index.stats["ms_build"], r["stats"]["ms_kernel"]))


def test_compare_clouds_is_the_host_comparison(eg3d_form):
    ctx, X = _resident(eg3d_form)
    rng = np.random.default_rng(77)
    md = float(F(0.01 * float(np.ptp(X[np.isfinite(X).all(axis=1)], axis=0).max())))
    ref = (X[::3] + rng.normal(0, 0.2 * md, X[::3].shape)).astype(F)
    ref_keep = (rng.uniform(size=len(ref)) < 0.9).astype(np.uint8)
    th = (md, 0.5 * md, 0.1 * md)
    got = ctx.compare_clouds(ref, md, thresholds=th, ref_keep=ref_keep)
    want = host.compare_clouds(X, ref, md, thresholds=th, ref_keep=ref_keep)
    for side in ("accuracy", "completeness"):
        for f in nc.FIGURES + ("mean", "median"):
            assert got[side][f] == want[side][f] or (got[side][f] != got[side][f] and want[side][f] != want[side][f]), (side, f)
        for f in nc.D2_FIGURES:
            assert F(got[side][f]).view(np.uint32) == F(want[side][f]).view(np.uint32), (side, f)
    assert 0 < got["accuracy"]["n_within"] < len(X) and got["completeness"]["n_within"] > 0


def test_the_device_outputs_feed_compact_device(eg3d_form):
    """The chain nearest_device -> a torch mask on the device buffer -> compact_device, in a child process of its own
    (tests/nearest_chain_child.py says why); EG3D_LIB, which the child inherits, is this form's library."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nearest_chain_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ok = [l for l in r.stdout.splitlines() if l.startswith("OK ")]
    assert len(ok) == 1 and 0 < int(ok[0].split()[2]) < int(ok[0].split()[1]), r.stdout


def test_refusals_leave_the_outputs_untouched(eg3d_form):
    ctx = _ctx(eg3d_form)
    case = nc.CASES[nc.IDS.index("one_cell")]
    n = len(case["X"])
    Xd = ctx.upload(case["X"])
    canary_d2, canary_nn = np.full(n, 7.5, F), np.full(n, 0xC0FFEE, np.uint32)
    d2d, nnd = ctx.upload(canary_d2), ctx.upload(canary_nn)
    other = ctx.clone()
    far = np.array([[0, 0, 0], [0, 0, 2097151.5]], F)

    def refused(code, call):
        with pytest.raises(api.Eg3dError) as e:
            call()
        assert e.value.code == code, (e.value.code, code, str(e.value))
        assert np.array_equal(d2d.numpy(F), canary_d2) and np.array_equal(nnd.numpy(np.uint32), canary_nn)

    try:
        with ctx.cloud_index(X=case["ref"], cell=0.25) as index, other.cloud_index(X=case["ref"], cell=0.25) as foreign:
            cloud = api.points_cloud(Xd, n)
            dev = lambda ix, md, th=(): (lambda: ctx.nearest_device(ix, md, cloud=cloud, thresholds=th, d2=d2d, nn=nnd))
            refused(api.ERR_NEAREST_MAXDIST, dev(index, 0.2500001))                 # max_dist > cell
            refused(api.ERR_NEAREST_MAXDIST, dev(index, 0.0))
            refused(api.ERR_NEAREST_FOREIGN, dev(foreign, 0.25))                    # an index of another context
            refused(api.ERR_NEAREST_THRESHOLD, dev(index, 0.25, (0.1,) * 9))        # nine thresholds
            refused(api.ERR_NEAREST_THRESHOLD, dev(index, 0.25, (0.3,)))
            incomplete = api.points_cloud(Xd, n)
            incomplete.complete = 0
            refused(-1, lambda: ctx.nearest_device(index, 0.25, cloud=incomplete, d2=d2d, nn=nnd))
            no_X = D.DeviceEdgePoints(n_points=n, complete=1)
            refused(-1, lambda: ctx.nearest_device(index, 0.25, cloud=no_X, d2=d2d, nn=nnd))
            # host outputs: the same rules, numpy canaries
            L, h2, hn = api.lib(), canary_d2.copy(), canary_nn.copy()
            st = D.nearest_stats_new((0.1,))
            rc = L.eg3d_cloud_nearest_points(ctx._h, D.np_ptr(case["X"], C.c_float), n, None, index._h, 0.26, D.np_ptr(h2, C.c_float),
                                             D.np_ptr(hn, C.c_uint32), C.byref(st))
            assert rc == api.ERR_NEAREST_MAXDIST and np.array_equal(h2, canary_d2) and np.array_equal(hn, canary_nn) and st.n_queries == 0
            # the index and the context work on
            nc.assert_same(ctx.nearest_points(index, case["X"], 0.25, thresholds=case["thresholds"]),
                           host.cloud_nearest(case["ref"], case["X"], 0.25, thresholds=case["thresholds"]), "after the refusals")
        # builds: an extent of 2^21 cells from two points, a bad cell; *index stays as it was
        for code, X, cell in ((api.ERR_NEAREST_EXTENT, far, 1.0), (api.ERR_NEAREST_CELL, far, 0.0), (api.ERR_NEAREST_CELL, far, float("nan"))):
            h = C.c_void_p(0x1234)
            st = D.CloudIndexStats(struct_size=C.sizeof(D.CloudIndexStats), n_cells=99)
            assert api.lib().eg3d_cloud_index_build(ctx._h, D.np_ptr(X, C.c_float), len(X), None, cell, C.byref(h), C.byref(st)) == code
            assert h.value == 0x1234 and st.n_cells == 99
        with ctx.cloud_index(X=np.array([[0, 0, 0], [0, 0, 2097150.5]], F), cell=1.0) as index:     # the largest extent accepted
            assert index.stats["dims"] == [1, 1, 2097151] and list(ctx.nearest_points(index, far, 0.5)[1]) == [0, api.NEAREST_NONE]
    finally:
        other.close()


def test_empty_inputs(eg3d_form):
    ctx = _ctx(eg3d_form)
    Q = np.random.default_rng(3).uniform(-1, 1, (70, 3)).astype(F)
    with ctx.cloud_index(X=np.zeros((0, 3), F), cell=0.5) as index:      # n_ref == 0: every query answers "none"
        assert index.n_indexed == 0 and index.n_cells == 0
        d2, nn, st = ctx.nearest_points(index, Q, 0.5, thresholds=(0.5,))
        assert np.isinf(d2).all() and (nn == api.NEAREST_NONE).all() and st["n_within"] == 0 and st["n_below"] == [0]
        assert np.isinf(st["min_d2"]) and np.isinf(st["max_d2"]) and np.isinf(st["median_d2"]) and st["sum_q32"] == 0
        d2, nn, st = ctx.nearest_points(index, np.zeros((0, 3), F), 0.5)
        assert len(d2) == 0 and st["n_queries"] == 0
    with ctx.cloud_index(X=Q, cell=0.5) as index:                        # n_queries == 0
        d2, nn, st = ctx.nearest_points(index, np.zeros((0, 3), F), 0.5, thresholds=(0.1,))
        assert len(d2) == 0 and len(nn) == 0 and st["n_queries"] == 0 and st["n_within"] == 0 and np.isinf(st["median_d2"])
        empty = D.DeviceEdgePoints(n_points=0, complete=1)
        assert ctx.nearest_device(index, 0.5, cloud=empty)["stats"]["n_queries"] == 0


def test_ownership_either_order(eg3d_form):
    """include/eg3d/nearest.hpp: an index is freed before or after its context is destroyed; neither order leaves an error
    or device memory behind."""
    base = _ctx(eg3d_form)
    Q = np.random.default_rng(4).uniform(-1, 1, (500, 3)).astype(F)
    want = host.cloud_nearest(Q, Q[:100] + F(0.01), 0.25)
    for index_first in (True, False):
        ctx = base.clone()
        index = ctx.cloud_index(X=Q, cell=0.25)
        nc.assert_same(ctx.nearest_points(index, Q[:100] + F(0.01), 0.25), want, "ownership")
        h = index._h
        if index_first:
            index.close()
            ctx.close()
        else:
            index._ctx = None
            ctx.close()
            api.lib().eg3d_cloud_index_free(h)
            index._h = C.c_void_p()
        assert api._hip().hipDeviceSynchronize() == 0
    # ... and the context the clones came from works on
    with base.cloud_index(X=Q, cell=0.25) as index:
        nc.assert_same(base.nearest_points(index, Q[:100] + F(0.01), 0.25), want, "after")
