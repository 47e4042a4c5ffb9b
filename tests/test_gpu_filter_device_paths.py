"""-m gpu: the branches of the filter stage on a device-resident cloud that a matched cloud never takes, on the hand-built
clouds of tests/filter_cloud_cases.py (tests/test_filter_cloud_cases.py shows with the oracle alone that they reach
them). k5_gn_filter<eg3d_off_t, false>: blocks that are not staged, staged and unstaged blocks in one launch, rigs of more
than 256 views (global-atomic histogram), the overflow bin, every bucket of the counting sort, keep masks over unstaged
and wholly masked blocks, device-side validation off the staged route. k6_compact_*: lists of 64 and more, empty lists,
a scan of more than 1024 block totals. k7_dedup_*: lists longer than a point's 8 lanes, empty lists.
Every comparison is bit for bit: Oracle.gn_filter, eg3d_host_observation_filter, cloudnp.np_compact,
eg3d_host_filter_close_2d."""
import ctypes as C

import numpy as np
import pytest

import filter_cloud_cases as fc
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host
from edgegraph3d_amd.cloudnp import np_compact, same_cloud
from edgegraph3d_amd.distributed import global_observation_threshold, observation_threshold

pytestmark = pytest.mark.gpu

_CTX = {}      # (form, rig) -> api.Context
_DEV = {}      # (form, case) -> (DeviceEdgePoints, DeviceArrays, host cloud dict)


@pytest.fixture(scope="module")
def have_gpu():
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"


def _ctx(form, c):
    """One context per DLT form and rig for the whole module (a rig of 256 / 257 views is not rebuilt per test)."""
    if (form, c.rig_id) not in _CTX:
        _CTX[(form, c.rig_id)] = api.Context(c.s.scene)
    return _CTX[(form, c.rig_id)]


def _dev(form, c):
    if (form, c.name) not in _DEV:
        _DEV[(form, c.name)] = fc.device_cloud(_ctx(form, c), c.X, c.off, c.view, c.xy)
    return _DEV[(form, c.name)]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    import forms
    _DEV.clear()
    for (rows, _), ctx in list(_CTX.items()):
        with forms.product_form(rows):   # eg3d_destroy of the library that created the context
            ctx.close()
    _CTX.clear()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_k5(ctx, c, dev, keep, legacy, X_out=None):
    """gn_filter_device on `dev` under the mask `keep` (numpy or None) against the oracle of the case."""
    Xr, ir = c.oracle(legacy)
    on = np.ones(c.n, bool) if keep is None else keep != 0
    kd = None if keep is None else ctx.upload(keep)
    Xd, inld, hist, n_inl, ms = ctx.gn_filter_device(dev, kd, c.mse, legacy, X_out=X_out)
    Xo, inl = Xd.numpy(np.float32, (c.n, 3)), inld.numpy(np.uint8)
    want_inl = np.where(on, ir, 0).astype(np.uint8)
    want_X = np.where(on[:, None], _bits(Xr), _bits(c.X))
    assert np.array_equal(inl, want_inl), np.flatnonzero(inl != want_inl)[:10]
    assert np.array_equal(_bits(Xo), want_X), np.flatnonzero((_bits(Xo) != want_X).any(axis=1))[:10]
    acc = want_inl != 0
    assert np.array_equal(hist, np.bincount(c.k[acc & (c.k <= c.V)], minlength=c.V + 1)), "hist[0..V]"
    assert n_inl == int(acc.sum())
    over = int((acc & (c.k > c.V)).sum())
    assert n_inl - int(hist.sum()) == over       # lists longer than the rig has views: counted, in no bin
    return acc, over, ms


@pytest.mark.parametrize("legacy", [False, True], ids=["abs", "legacy abs"])
@pytest.mark.parametrize("name", fc.K5_CASES)
def test_k5_against_the_oracle(have_gpu, eg3d_form, name, legacy):
    c = fc.case(name)
    ctx = _ctx(eg3d_form, c)
    dev, _, _ = _dev(eg3d_form, c)
    acc, over, ms = _check_k5(ctx, c, dev, None, legacy)
    print("%s; legacy %d, kernel %.3f ms" % (c.coverage(acc), legacy, ms))
    assert over >= 4 and acc.any() and not acc.all()


@pytest.mark.parametrize("mask", fc.MASKS)
@pytest.mark.parametrize("name", ["rig16", "rig257"])
def test_k5_masks(have_gpu, eg3d_form, name, mask):
    c = fc.case(name)
    ctx = _ctx(eg3d_form, c)
    dev, _, _ = _dev(eg3d_form, c)
    keep = fc.mask(c, mask)
    acc, over, _ = _check_k5(ctx, c, dev, keep, False)
    print("%s; mask %s keeps %d points: %d inliers, overflow bin %d" % (c.coverage(), mask, keep.sum(), acc.sum(), over))
    assert acc.any() == (mask != "zeros")


def test_k5_x_out_may_alias_x(have_gpu, eg3d_form):
    c = fc.case("rig16")
    ctx = _ctx(eg3d_form, c)
    dev, _, _ = _dev(eg3d_form, c)
    Xa = ctx.upload(c.X)          # a copy of X: the case's cloud stays as it is
    alias = fc.same_view(dev)
    alias.X = Xa.ptr
    acc, over, _ = _check_k5(ctx, c, alias, fc.mask(c, "random50"), False, X_out=Xa)
    print("%s; in place under mask random50: %d inliers, overflow bin %d" % (c.coverage(), acc.sum(), over))


def test_threshold_and_compaction_end_to_end(have_gpu, eg3d_form):
    c = fc.case("threshold16")
    ctx = _ctx(eg3d_form, c)
    dev, _, cloud = _dev(eg3d_form, c)
    Xr, ir = c.oracle(False)
    thr, surv = fc.host_threshold(c.V, c.k, ir)
    Xd, inld, hist, n_inl, _ = ctx.gn_filter_device(dev, None, c.mse, False)
    got_thr = observation_threshold(hist, c.V, -1, count=n_inl)
    print("%s; hist %s, n_inliers %d, threshold %d (host %d)" % (c.coverage(ir), hist.tolist(), n_inl, got_thr, thr))
    assert got_thr == thr
    assert global_observation_threshold(None, hist, c.V, -1, None, local_count=n_inl) == thr   # filter_then_gather's route
    assert thr > 3
    assert n_inl == int(ir.sum()) > hist.sum()
    out = ctx.compact_device(dev, inld, Xd, got_thr)
    want = np_compact(cloud, surv, Xr)
    assert 0 < want["n_points"] < int(ir.sum())
    assert same_cloud(ctx.fetch_device_points(out, 0, int(out.n_points)), want) is None


def _check_compaction(ctx, dev, cloud, keep, X_new, min_obs, keep_dev=None, X_dev=None):
    out = ctx.compact_device(dev, keep_dev if keep is not None else None, X_dev if X_new is not None else None, min_obs)
    assert out.complete == 1
    want = np_compact(cloud, np.ones(cloud["n_points"], np.uint8) if keep is None else keep, X_new, min_obs)
    assert (int(out.n_points), int(out.n_obs)) == (want["n_points"], want["n_obs"]), ("totals", min_obs)
    bad = same_cloud(ctx.fetch_device_points(out, 0, int(out.n_points)), want)
    assert bad is None, (bad, min_obs)
    return want


@pytest.mark.parametrize("name", ["rig16", "rig257"])
def test_k6_long_and_empty_lists(have_gpu, eg3d_form, name):
    c = fc.case(name)
    ctx = _ctx(eg3d_form, c)
    dev, _, cloud = _dev(eg3d_form, c)
    Xn = np.random.default_rng(6).standard_normal((c.n, 3)).astype(np.float32)
    Xn_dev = ctx.upload(Xn)
    keeps = [("none", None)] + [(m, fc.mask(c, m)) for m in fc.MASKS]
    lone = fc.lone_empty_between_long(c)
    if name == "rig16":
        assert lone is not None
        keeps.append(("lone empty list", lone))
    sizes = []
    for kn, keep in keeps:
        kd = None if keep is None else ctx.upload(keep)
        for min_obs in (-1, 0, 3, 64):
            for X_new in (None, Xn):
                w = _check_compaction(ctx, dev, cloud, keep, X_new, min_obs, kd, Xn_dev)
            sizes.append("%s/%d: %d points %d obs" % (kn, min_obs, w["n_points"], w["n_obs"]))
    print("%s; survivors by keep / min_obs: %s" % (c.coverage(), "; ".join(sizes)))
    if name == "rig16":
        w = _check_compaction(ctx, dev, cloud, lone, None, -1, ctx.upload(lone))
        assert w["n_points"] == 3 and w["obs_off"][1] == w["obs_off"][2] >= 64 and w["n_obs"] >= 128
        assert _check_compaction(ctx, dev, cloud, None, None, -1)["n_points"] == c.n        # empty lists survive min_obs < 0
        assert _check_compaction(ctx, dev, cloud, None, None, 0)["n_points"] == int((c.k > 0).sum())
    assert _check_compaction(ctx, dev, cloud, None, None, 64)["n_points"] == int((c.k > 64).sum()) > 0


@pytest.mark.parametrize("n", [fc.K6_SCAN_TRIP, fc.K6_SCAN_TRIP + 3 * 256 + 5], ids=["one trip exactly", "a second trip"])
def test_k6_scan_beyond_one_trip(have_gpu, eg3d_form, n):
    """k6_compact_scan carries base_p / base_o from one trip of 1024 block totals to the next. With more than 1024 blocks
    the blocks of the second trip get their destination from the carry: without base_p their points land at the front of
    the output (X, key, obs_off of the survivors differ), without base_o their observations do and their obs_off restart at
    0; the totals n_points / n_obs are the carry after the last trip."""
    c = fc.case("rig16")
    ctx = _ctx(eg3d_form, c)       # (any context: the compaction does not look at the rig)
    dev, arrays, cloud = fc.device_cloud(ctx, *fc.scan_cloud(n))
    rng = np.random.default_rng(70)
    keep = (rng.random(n) < 0.7).astype(np.uint8)
    Xn = rng.standard_normal((n, 3)).astype(np.float32)
    kd, xd = ctx.upload(keep), ctx.upload(Xn)
    for min_obs in (-1, 1):
        w = _check_compaction(ctx, dev, cloud, keep, Xn, min_obs, kd, xd)
        tail = np_compact(cloud, keep * (np.arange(n) >= fc.K6_SCAN_TRIP), Xn, min_obs)
        print("scan cloud %d points / %d blocks, min_obs %d: %d points %d obs survive, %d / %d of them from blocks of a second trip"
              % (n, (n + 255) // 256, min_obs, w["n_points"], w["n_obs"], tail["n_points"], tail["n_obs"]))
        assert w["n_points"] > fc.K6_SCAN_TRIP // 4
        assert (tail["n_points"] > 0 and tail["n_obs"] > 0) == (n > fc.K6_SCAN_TRIP)


def _refused(rc, text):
    return rc != 0 and text in api.lib().eg3d_last_error()


@pytest.mark.parametrize("name", ["rig16", "rig257"])
def test_malformed_input_off_the_staged_route(have_gpu, eg3d_form, name):
    """A view id out of range and a descending offset pair in a block that is NOT staged (rig16: the heavy block; rig257:
    the light block of a rig too wide to stage). Every bad value lies inside what the buffers hold."""
    c = fc.case(name)
    L, ctx = api.lib(), _ctx(eg3d_form, c)
    dev, _, cloud = _dev(eg3d_form, c)
    b = c.first_heavy() if name == "rig16" else c.first_light()
    assert not c.staged[b]
    p0 = b * 256
    i = p0 + 100 + int(np.flatnonzero(c.k[p0 + 100:p0 + 200] >= 2)[0])      # a point in the middle of the block, a list of >= 2
    Xd, inld, out = ctx.device_alloc(12 * c.n), ctx.device_alloc(c.n), D.DeviceEdgePoints()
    print("%s; bad values at point %d (list of %d) of block %d, which is not staged" % (c.coverage(), i, c.k[i], b))

    def filter_rc(d):
        return L.eg3d_gn_filter_device(ctx._h, C.byref(d), None, c.mse, 0, Xd.ptr, inld.ptr, None, None, None)

    for v in (c.V, -1):
        view = c.view.copy()
        view[int(c.off[i]) + 1] = v
        vd = ctx.upload(view)
        bad = fc.same_view(dev)
        bad.obs_view = vd.ptr
        assert _refused(filter_rc(bad), b"view id out of range"), v
    off = cloud["obs_off"][:c.n].copy()
    assert 0 < off[i] < off[i + 1] <= c.n_obs
    swapped = off.copy()
    swapped[[i, i + 1]] = off[[i + 1, i]]                 # two neighbouring in-range offsets, swapped
    lowered = off.copy()
    j = i - 1 - int(np.flatnonzero(c.k[:i][::-1] > 0)[0])
    lowered[i + 1] = off[j]                               # an offset lowered to an earlier in-range value
    assert lowered[i + 1] < lowered[i]
    for o in (swapped, lowered):
        assert o.max() <= c.n_obs
        od = ctx.upload(o)
        bad = fc.same_view(dev)
        bad.obs_off = od.ptr
        assert _refused(filter_rc(bad), b"obs_off")
        assert _refused(L.eg3d_compact_device(ctx._h, C.byref(bad), None, None, -1, C.byref(out)), b"obs_off")
    # ... and the context still works afterwards
    _check_k5(ctx, c, dev, fc.mask(c, "random50"), False)
    _check_compaction(ctx, dev, cloud, None, None, 3)


def test_dedup_of_long_and_empty_lists(have_gpu, eg3d_form):
    c = fc.case("rig16")
    ctx = _ctx(eg3d_form, c)
    dev, _, cloud = _dev(eg3d_form, c)
    sc = c.s.scene.contents
    ep = D.EdgePointsArrays(cloud)
    want = np.zeros(c.n, np.uint8)
    assert host.lib().eg3d_host_filter_close_2d(c.V, int(sc.width), int(sc.height), C.byref(ep.c), D.np_ptr(want, C.c_uint8)) == 0
    keep, n_kept = ctx.dedup_device(dev)
    got = keep.numpy(np.uint8)
    print("%s; dedup keeps %d, drops %d with observations" % (c.coverage(), n_kept, ((want == 0) & (c.k > 0)).sum()))
    assert 0 < want.sum() < c.n and not want[c.k == 0].any()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert n_kept == int(want.sum())
