"""-m gpu: the filter stage on a device-resident cloud (eg3d_gn_filter_device, eg3d_compact_device,
eg3d_filter_resident). Every device result is compared bit for bit: the Gauss-Newton verdicts and positions with the
CPU oracle on the fetched cloud, the threshold with eg3d_host_observation_filter, the compaction with a numpy
compaction of the fetched cloud (all seven arrays, in order)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host
from edgegraph3d_amd.cloudnp import np_compact, same_cloud

pytestmark = pytest.mark.gpu

_CACHE = {}


def _oracle(scene):
    from oracle import binding as ob
    return ob.Oracle(scene)


class _C2:
    """The C2 cloud of one DLT form, left in HBM by a device-only match, its host copy and the oracle's filter results."""

    def __init__(self, rows):
        assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
        self.s = host.Synth(2)
        self.ctx = api.Context(self.s.scene)
        r = self.ctx.match_refpoints(self.s.seeds, device_only=True)
        self.dev = self.ctx.last_device_output()
        assert self.dev.complete == 1 and int(self.dev.n_points) == r["n_points"] > 1000
        self.cloud = self.ctx.fetch_device_output()
        self.n = self.cloud["n_points"]
        self.k = np.diff(self.cloud["obs_off"].astype(np.int64))
        self.V = self.s.n_views
        self.ref = {}
        # 2.25 is the reference's default. The checks below need both verdicts and some moved X; the 6x4 cloud has them at
        # 2.25 (96.3 % inliers). Should the 4x4 form's cloud lack either there, it is filtered at 0.1, a bound tight enough
        # to reject a good share of any cloud matched from noisy observations (85.8 % inliers on the 6x4 one).
        self.mse = 2.25
        Xr, ir = self.oracle(2.25, False)
        if rows == 2 and (ir.all() or not ir.any() or np.array_equal(Xr.view(np.uint32), self.cloud["X"].view(np.uint32))):
            self.mse = 0.1

    def oracle(self, mse, legacy, cloud=None):
        key = (mse, bool(legacy))
        if cloud is not None:
            return _oracle(self.s.scene).gn_filter(cloud["X"], cloud["obs_off"].astype(np.uint32), cloud["obs_view"],
                                                   cloud["obs_xy"], mse, legacy_abs=legacy, nthreads=16)
        if key not in self.ref:
            c = self.cloud
            self.ref[key] = _oracle(self.s.scene).gn_filter(c["X"], c["obs_off"].astype(np.uint32), c["obs_view"], c["obs_xy"],
                                                            mse, legacy_abs=legacy, nthreads=16)
        return self.ref[key]

    def view(self, n):
        """The first n points as a caller-built device view."""
        d = D.DeviceEdgePoints()
        C.memmove(C.byref(d), C.byref(self.dev), C.sizeof(d))
        d.n_points, d.n_obs = n, int(self.cloud["obs_off"][n])
        return d


@pytest.fixture
def c2(eg3d_form):
    if eg3d_form not in _CACHE:
        _drop_cache()   # (the other form's context belongs to a library that is no longer the selected one)
        _CACHE[eg3d_form] = _C2(eg3d_form)
    return _CACHE[eg3d_form]


def _drop_cache():
    import forms
    for rows, c in list(_CACHE.items()):
        with forms.product_form(rows):   # eg3d_destroy of the library that created the context
            c.ctx.close()
    _CACHE.clear()


@pytest.fixture(scope="module", autouse=True)
def _close_cached_contexts():
    yield
    _drop_cache()


def _host_threshold(V, k, inl, forced, sfm_k=None):
    """eg3d_host_observation_filter on [SfM points] + [the cloud]: (threshold, surviving mask of the cloud)."""
    sfm_k = np.zeros(0, np.int64) if sfm_k is None else sfm_k
    off = np.concatenate([[0], np.cumsum(np.concatenate([sfm_k, k]))]).astype(np.uint32)
    mask = np.concatenate([np.ones(len(sfm_k), np.uint8), np.asarray(inl, np.uint8)])
    thr = host.lib().eg3d_host_observation_filter(V, D.np_ptr(off, C.c_uint32), len(mask), len(sfm_k), forced,
                                                  D.np_ptr(mask, C.c_uint8))
    return thr, mask[len(sfm_k):]


@pytest.mark.parametrize("legacy", [False, True], ids=["abs", "legacy abs"])
def test_c2_cloud_against_the_oracle(c2, legacy):
    Xr, ir = c2.oracle(c2.mse, legacy)
    Xd, inld, hist, n_inl, ms = c2.ctx.gn_filter_device(c2.dev, None, c2.mse, legacy)
    Xo, inl = Xd.numpy(np.float32, (c2.n, 3)), inld.numpy(np.uint8)
    moved = (Xr.view(np.uint32) != c2.cloud["X"].view(np.uint32)).any(axis=1)
    print("C2 %d points, k %d..%d, mse %.2f legacy %d: inliers %.4f, X moved on %.4f of the inliers, kernel %.3f ms"
          % (c2.n, c2.k.min(), c2.k.max(), c2.mse, legacy, ir.mean(), moved[ir != 0].mean(), ms))
    assert ir.any() and not ir.all(), "both verdicts must occur"
    assert moved.any(), "some X must move"
    assert np.array_equal(inl, ir)
    assert np.array_equal(Xo.view(np.uint32), Xr.view(np.uint32))
    assert np.array_equal(hist, np.bincount(c2.k[ir != 0], minlength=c2.V + 1)[:c2.V + 1])
    assert hist.sum() == int(((ir != 0) & (c2.k <= c2.V)).sum())   # lists longer than the rig has views sit in no bin
    assert n_inl == int(ir.sum())                                  # ... but are counted
    # X_out may alias the cloud's X: the same result in place (on a copy of X, the cloud itself stays as matched)
    Xa = c2.ctx.upload(c2.cloud["X"])
    alias = c2.view(c2.n)
    alias.X = Xa.ptr
    c2.ctx.gn_filter_device(alias, None, c2.mse, legacy, X_out=Xa, inlier=inld)
    assert np.array_equal(Xa.numpy(np.uint32), Xr.view(np.uint32).ravel()) and np.array_equal(inld.numpy(np.uint8), ir)


def test_mask(c2):
    Xr, ir = c2.oracle(c2.mse, False)
    keep = (np.random.default_rng(7).random(c2.n) < 0.5).astype(np.uint8)
    Xd, inld, hist, n_inl, _ = c2.ctx.gn_filter_device(c2.dev, c2.ctx.upload(keep), c2.mse, False)
    Xo, inl = Xd.numpy(np.float32, (c2.n, 3)), inld.numpy(np.uint8)
    off, on = keep == 0, keep != 0
    assert off.sum() > 1000 and on.sum() > 1000
    assert not inl[off].any()
    assert np.array_equal(Xo[off].view(np.uint32), c2.cloud["X"][off].view(np.uint32))
    assert np.array_equal(inl[on], ir[on]) and np.array_equal(Xo[on].view(np.uint32), Xr[on].view(np.uint32))
    assert np.array_equal(hist, np.bincount(c2.k[on & (ir != 0)], minlength=c2.V + 1)[:c2.V + 1])
    assert n_inl == int((on & (ir != 0)).sum())


def _check_compaction(c2, dev, cloud, keep, X_new, min_obs):
    out = c2.ctx.compact_device(dev, None if keep is None else c2.ctx.upload(keep), None if X_new is None else c2.ctx.upload(X_new),
                                min_obs)
    assert out.complete == 1
    got = c2.ctx.fetch_device_points(out, 0, int(out.n_points))
    want = np_compact(cloud, np.ones(cloud["n_points"], np.uint8) if keep is None else keep, X_new, min_obs)
    bad = same_cloud(got, want)
    assert bad is None, (bad, min_obs)
    return want


def test_compaction_masks(c2):
    n, cloud = c2.n, c2.cloud
    rng = np.random.default_rng(3)
    Xn = rng.standard_normal((n, 3)).astype(np.float32)
    none = _check_compaction(c2, c2.dev, cloud, np.zeros(n, np.uint8), None, -1)
    assert none["n_points"] == 0 and none["n_obs"] == 0
    everything = _check_compaction(c2, c2.dev, cloud, None, None, -1)
    assert same_cloud(everything, cloud) is None
    everything = _check_compaction(c2, c2.dev, cloud, np.ones(n, np.uint8), Xn, -1)
    assert everything["n_points"] == n and np.array_equal(everything["X"], Xn)
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[0], last[-1] = 1, 1
    assert _check_compaction(c2, c2.dev, cloud, first, None, -1)["n_points"] == 1
    assert _check_compaction(c2, c2.dev, cloud, last, Xn, -1)["n_points"] == 1
    _check_compaction(c2, c2.dev, cloud, (np.arange(n) % 2).astype(np.uint8), None, -1)
    _check_compaction(c2, c2.dev, cloud, (np.arange(n) % 2 == 0).astype(np.uint8), Xn, 3)
    _check_compaction(c2, c2.dev, cloud, (rng.random(n) < 0.03).astype(np.uint8), None, -1)  # sparse: whole waves without a survivor


def test_compaction_min_obs(c2):
    sizes = []
    for m in range(2, 10):
        sizes.append(_check_compaction(c2, c2.dev, c2.cloud, None, None, m)["n_points"])
    assert sizes[0] > sizes[-1] and sorted(sizes, reverse=True) == sizes, sizes


def test_compaction_of_a_point_count_that_is_no_multiple_of_64_or_256(c2):
    for n in (256 * 40 + 64 + 37, 63, 1):
        assert n % 64 and n % 256 and n < c2.n
        sub = {"n_points": n, "n_obs": int(c2.cloud["obs_off"][n]), "X": c2.cloud["X"][:n], "obs_off": c2.cloud["obs_off"][:n + 1],
               "key": c2.cloud["key"][:n]}
        for name in ("obs_view", "obs_pl", "obs_seg", "obs_xy"):
            sub[name] = c2.cloud[name][:sub["n_obs"]]
        keep = (np.random.default_rng(n).random(n) < 0.7).astype(np.uint8)
        keep[-1] = 1
        _check_compaction(c2, c2.view(n), sub, keep, None, 3)
        _check_compaction(c2, c2.view(n), sub, None, None, -1)


def test_compaction_of_a_concatenated_cloud(c2):
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "filter_resident_concat_check.py")], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "CONCAT-COMPACT-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("forced", [-1, 4])
@pytest.mark.parametrize("with_base", [False, True], ids=["no base_hist", "base_hist"])
@pytest.mark.parametrize("to_host", [True, False], ids=["to host", "device only"])
def test_filter_resident_end_to_end(c2, to_host, with_base, forced):
    # (c2.ctx's last device output is still the C2 cloud: the filter and the compaction have buffers of their own)
    Xr, ir = c2.oracle(c2.mse, False)
    sfm_k = np.random.default_rng(9).integers(2, c2.V + 1, 50000).astype(np.int64) if with_base else None
    thr, surv = _host_threshold(c2.V, c2.k, ir, forced, sfm_k)
    want = np_compact(c2.cloud, surv, Xr)
    base = np.bincount(sfm_k, minlength=c2.V + 1).astype(np.uint64) if with_base else None
    got, dev, st = c2.ctx.filter_resident(c2.mse, False, forced, base, to_host)
    print("filter_resident: threshold %d, %d -> %d inliers -> %d kept; filter %.3f ms, compact %.3f ms, copy %.3f ms"
          % (st["threshold"], st["n_points_in"], st["n_gn_inliers"], st["n_kept"], st["ms_filter"], st["ms_compact"], st["ms_copy"]))
    assert st["threshold"] == thr
    assert st["n_points_in"] == st["n_masked_in"] == c2.n and st["n_gn_inliers"] == int(ir.sum())
    assert st["n_kept"] == want["n_points"] and st["n_obs_kept"] == want["n_obs"] and 0 < want["n_points"] < c2.n
    assert st["struct_size"] == C.sizeof(D.FilterStats)
    assert same_cloud(c2.ctx.fetch_device_points(dev, 0, int(dev.n_points)), want) is None
    if to_host:
        assert same_cloud(got, want) is None
        assert int(got["obs_off"][-1]) == want["n_obs"]   # the sentinel
    else:
        assert got is None


def test_reference_order_dedup_mask_then_filter(c2):
    """The reference dedups before it filters: host dedup mask as keep_dev, then the compaction of mask AND inlier above
    the threshold == the filter applied to the host-compacted deduplicated cloud."""
    sc = c2.s.scene.contents
    ep = D.EdgePointsArrays(c2.cloud)
    dedup = np.zeros(c2.n, np.uint8)
    assert host.lib().eg3d_host_filter_close_2d(c2.V, int(sc.width), int(sc.height), C.byref(ep.c), D.np_ptr(dedup, C.c_uint8)) == 0
    assert 0 < dedup.sum() < c2.n
    small = np_compact(c2.cloud, dedup)
    Xs, inls = c2.oracle(c2.mse, False, cloud=small)
    thr, surv = _host_threshold(c2.V, np.diff(small["obs_off"].astype(np.int64)), inls, -1)
    want = np_compact(small, surv, Xs)
    Xd, inld, hist, n_inl, _ = c2.ctx.gn_filter_device(c2.dev, c2.ctx.upload(dedup), c2.mse, False)
    from edgegraph3d_amd.distributed import observation_threshold
    assert n_inl == int(inld.numpy(np.uint8).sum())
    assert observation_threshold(hist, c2.V, -1, count=n_inl) == thr
    out = c2.ctx.compact_device(c2.dev, inld, Xd, thr)
    assert 0 < want["n_points"] < small["n_points"]
    assert same_cloud(c2.ctx.fetch_device_points(out, 0, int(out.n_points)), want) is None


class _OneRankGather:
    """distributed.filter_then_gather's `gather` on one rank: the exchange returns the rank's own shard."""

    def allgather(self, local_dev):
        return local_dev, 0


@pytest.mark.parametrize("forced", [-1, 4])
def test_filter_then_gather_on_one_rank(c2, forced):
    """The multi-rank glue without a process group (dist = None) and with a gather that hands the shard back: per-rank
    filter, threshold from the histogram and the inlier count, compaction — the cloud filter_resident gives."""
    from edgegraph3d_amd.distributed import filter_then_gather
    Xr, ir = c2.oracle(c2.mse, False)
    thr, surv = _host_threshold(c2.V, c2.k, ir, forced)
    want = np_compact(c2.cloud, surv, Xr)
    out, rc, got_thr = filter_then_gather(c2.ctx, _OneRankGather(), None, c2.mse, False, forced)
    assert rc == 0 and got_thr == thr
    assert same_cloud(c2.ctx.fetch_device_points(out, 0, int(out.n_points)), want) is None
    # with a mask of the shard (its dedup mask, say): masked points never pass
    keep = (np.random.default_rng(21).random(c2.n) < 0.5).astype(np.uint8)
    out, rc, _ = filter_then_gather(c2.ctx, _OneRankGather(), None, c2.mse, False, 3, keep=c2.ctx.upload(keep))
    assert rc == 0
    want = np_compact(c2.cloud, (keep != 0) & (ir != 0), Xr, 3)
    assert same_cloud(c2.ctx.fetch_device_points(out, 0, int(out.n_points)), want) is None


def test_errors(c2, monkeypatch):
    L, ctx = api.lib(), c2.ctx
    h = ctx._h
    dev = c2.view(c2.n)
    out = D.DeviceEdgePoints()
    Xd, inld = ctx.device_alloc(12 * c2.n), ctx.device_alloc(c2.n)

    def refused(rc):
        return rc == -1 and len(L.eg3d_last_error()) > 0

    assert refused(L.eg3d_gn_filter_device(h, None, None, 2.25, 0, Xd.ptr, inld.ptr, None, None, None))
    assert refused(L.eg3d_gn_filter_device(None, C.byref(dev), None, 2.25, 0, Xd.ptr, inld.ptr, None, None, None))
    assert refused(L.eg3d_gn_filter_device(h, C.byref(dev), None, 2.25, 0, None, inld.ptr, None, None, None))
    assert refused(L.eg3d_gn_filter_device(h, C.byref(dev), None, 2.25, 0, Xd.ptr, None, None, None, None))
    assert refused(L.eg3d_compact_device(h, None, None, None, -1, C.byref(out)))
    assert refused(L.eg3d_compact_device(h, C.byref(dev), None, None, -1, None))
    assert refused(L.eg3d_compact_device(h, C.byref(dev), None, None, -1, C.byref(dev)))   # out aliases cloud
    assert b"alias" in L.eg3d_last_error()
    assert refused(L.eg3d_filter_resident(None, 2.25, 0, -1, None, 0, None, None, None))
    assert refused(L.eg3d_filter_resident(h, 2.25, 0, -1, None, 1, None, None, None))      # to_host without out_host
    st = D.FilterStats()
    st.struct_size = C.sizeof(D.FilterStats) - 4
    st.n_kept = 12345
    assert refused(L.eg3d_filter_resident(h, 2.25, 0, -1, None, 0, None, None, C.byref(st)))
    assert b"struct_size" in L.eg3d_last_error() and st.n_kept == 12345                     # nothing written
    # an incomplete view: by hand, and as a host-copy call that ran in several sub-batches leaves it
    part = c2.view(c2.n)
    part.complete = 0
    assert refused(L.eg3d_gn_filter_device(h, C.byref(part), None, 2.25, 0, Xd.ptr, inld.ptr, None, None, None))
    assert refused(L.eg3d_compact_device(h, C.byref(part), None, None, -1, C.byref(out)))
    s1 = host.Synth(1)
    monkeypatch.setenv("EG3D_MAX_SCRATCH_MB", "48")     # read once, when a context is created: config 1 then takes several chunks
    other = api.Context(s1.scene)
    monkeypatch.delenv("EG3D_MAX_SCRATCH_MB")
    other.match_refpoints(s1.seeds)
    assert other.last_device_output().complete == 0
    assert refused(L.eg3d_filter_resident(other._h, 2.25, 0, -1, None, 0, None, C.byref(out), None))
    assert b"complete" in L.eg3d_last_error()
    other.close()
    # a view id out of range fails the call (device-side check), whichever block holds it
    view = c2.cloud["obs_view"].copy()
    view[len(view) // 2] = c2.V
    bad = c2.view(c2.n)
    vd = ctx.upload(view)
    bad.obs_view = vd.ptr
    rc = L.eg3d_gn_filter_device(h, C.byref(bad), None, 2.25, 0, Xd.ptr, inld.ptr, None, None, None)
    assert rc != 0 and b"view id out of range" in L.eg3d_last_error()
    view[len(view) // 2] = -1
    vd2 = ctx.upload(view)   # (held in a name: a DeviceArray frees its memory when it is collected)
    bad.obs_view = vd2.ptr
    assert L.eg3d_gn_filter_device(h, C.byref(bad), None, 2.25, 0, Xd.ptr, inld.ptr, None, None, None) != 0
    # offsets that do not ascend fail it too (nothing is read through them)
    off = c2.cloud["obs_off"][:-1].copy()
    off[c2.n // 3] = off[c2.n // 3 + 1] + 5
    bad = c2.view(c2.n)
    od = ctx.upload(off)
    bad.obs_off = od.ptr
    assert L.eg3d_gn_filter_device(h, C.byref(bad), None, 2.25, 0, Xd.ptr, inld.ptr, None, None, None) != 0
    assert b"obs_off" in L.eg3d_last_error()
    assert L.eg3d_compact_device(h, C.byref(bad), None, None, -1, C.byref(out)) != 0
    # ... and the context still works afterwards
    test_mask(c2)
