"""-m gpu: the 3 px dedup on a device-resident cloud (eg3d_dedup_device, eg3d_dedup_resident). Every mask is compared
byte for byte with eg3d_host_filter_close_2d and orc_filter_close_2d on the fetched cloud, every cloud bit for bit with a
numpy compaction (all seven arrays, in order)."""
import ctypes as C

import numpy as np
import pytest

import dedup_cases as dc
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host
from edgegraph3d_amd.cloudnp import np_compact, np_dedup, same_cloud
from dedup_gpu_cases import C2Cloud, host_threshold

pytestmark = pytest.mark.gpu

_CACHE = {}


def _drop_cache():
    import forms
    for rows, c in list(_CACHE.items()):
        with forms.product_form(rows):
            c.ctx.close()
    _CACHE.clear()


@pytest.fixture
def c2(eg3d_form):
    if eg3d_form not in _CACHE:
        _drop_cache()
        _CACHE[eg3d_form] = C2Cloud(eg3d_form)
    return _CACHE[eg3d_form]


@pytest.fixture(scope="module", autouse=True)
def _close_cached_contexts():
    yield
    _drop_cache()


def test_c2_cloud_against_host_and_oracle(c2):
    from oracle import binding as ob
    keep, n_kept = c2.ctx.dedup_device(c2.dev)
    got = keep.numpy(np.uint8)
    print("C2: %d of %d points kept by the dedup" % (n_kept, c2.n))
    assert np.array_equal(got, c2.dedup)
    assert np.array_equal(got, dc.oracle_mask(ob.Oracle(c2.s.scene), c2.cloud))
    assert np.array_equal(got, np_dedup(c2.cloud, c2.V, c2.W, c2.H))
    assert n_kept == int(got.sum()) and 0 < n_kept < c2.n
    # the same call again gives the same mask (reset), and without a reset every cell is already claimed by these indices
    again, n2 = c2.ctx.dedup_device(c2.dev, keep=keep)
    assert n2 == n_kept and np.array_equal(again.numpy(np.uint8), c2.dedup)
    same, n3 = c2.ctx.dedup_device(c2.dev, reset=False)
    assert n3 == n_kept and np.array_equal(same.numpy(np.uint8), c2.dedup)


def test_prefix_views(c2):
    for n in (0, 1, 63, 64, 65, c2.n - 1):
        keep, n_kept = c2.ctx.dedup_device(c2.view(n))
        got = keep.numpy(np.uint8)[:n]
        assert np.array_equal(got, c2.dedup[:n]), n     # the mask of a prefix is the prefix of the mask
        assert n_kept == int(c2.dedup[:n].sum()), n


def test_claims_across_calls(c2):
    n_seeds = int(c2.s.seeds.contents.n_seeds)
    cuts = [0, n_seeds // 3, n_seeds // 2, n_seeds]
    ctx = api.Context(c2.s.scene)
    try:
        masks, parts, base = [], [], 0
        for b, e in zip(cuts[:-1], cuts[1:]):
            r = ctx.match_refpoints(c2.s.seeds, b, e, device_only=True)
            dev = ctx.last_device_output()
            assert dev.complete == 1 and r["n_points"] > 1000
            parts.append(ctx.fetch_device_output())
            keep, n_kept = ctx.dedup_device(dev, index_base=base, reset=(base == 0))
            masks.append(keep.numpy(np.uint8))
            assert n_kept == int(masks[-1].sum())
            base += int(dev.n_points)
        assert base == c2.n
        whole = dc.concat_clouds(dc.concat_clouds(parts[0], parts[1]), parts[2])
        assert same_cloud(whole, c2.cloud) is None
        assert np.array_equal(np.concatenate(masks), c2.dedup)
        # a reset in the middle: the last part deduplicated alone, as the host does on that part
        dev = ctx.last_device_output()
        alone, _ = ctx.dedup_device(dev, index_base=base - int(dev.n_points), reset=True)
        alone = alone.numpy(np.uint8)
        assert np.array_equal(alone, dc.host_mask(parts[2], c2.V, c2.W, c2.H))
        assert not np.array_equal(alone, masks[2]) and alone.sum() > masks[2].sum()
    finally:
        ctx.close()


def _upload_cloud(ctx, cloud):
    arrays = {"X": cloud["X"], "obs_off": cloud["obs_off"][:-1], "obs_view": cloud["obs_view"], "obs_pl": cloud["obs_pl"],
              "obs_seg": cloud["obs_seg"], "obs_xy": cloud["obs_xy"], "key": cloud["key"]}
    held = {k: ctx.upload(v) for k, v in arrays.items()}
    d = D.DeviceEdgePoints()
    d.n_points, d.n_obs, d.complete = int(cloud["n_points"]), int(cloud["n_obs"]), 1
    for k, a in held.items():
        setattr(d, k, a.ptr)
    return d, held


def test_hostile_clouds(eg3d_form):
    V, W, H = dc.HOSTILE_RIG
    s = host.Synth(1)
    sc = dc.scene_with_size(s.scene, W, H)
    ctx = api.Context(C.byref(sc))
    try:
        assert ctx.n_views == V
        for name, (cloud, trivial) in dc.hostile_clouds().items():
            want = dc.host_mask(cloud, V, W, H)
            d, held = _upload_cloud(ctx, cloud)
            keep, n_kept = ctx.dedup_device(d)     # (no error for off-image or out-of-rig observations)
            got = keep.numpy(np.uint8)[:len(want)]
            assert np.array_equal(got, want), name
            assert n_kept == int(want.sum()), name
            assert trivial or (want.any() and not want.all()), name
            # in two calls over persistent claims
            n = len(want)
            cut = n // 2
            a, b = dc.slice_cloud(cloud, 0, cut), dc.slice_cloud(cloud, cut, n)
            da, ha = _upload_cloud(ctx, a)
            db, hb = _upload_cloud(ctx, b)
            ka, _ = ctx.dedup_device(da, 0, True)
            kb, _ = ctx.dedup_device(db, cut, False)
            assert np.array_equal(np.concatenate([ka.numpy(np.uint8)[:cut], kb.numpy(np.uint8)[:n - cut]]), want), name
    finally:
        ctx.close()


def test_offsets_that_do_not_ascend_are_an_argument_error(c2):
    L, ctx = api.lib(), c2.ctx
    keep = ctx.device_alloc(c2.n)
    for where, value in ((c2.n // 3, None), (c2.n - 1, int(c2.cloud["n_obs"]) + 1)):
        off = c2.cloud["obs_off"][:-1].copy()
        off[where] = off[where + 1] + 5 if value is None else value
        bad = c2.view(c2.n)
        od = ctx.upload(off)
        bad.obs_off = od.ptr
        assert L.eg3d_dedup_device(ctx._h, C.byref(bad), 0, 1, keep.ptr, None) == -1
        assert b"obs_off" in L.eg3d_last_error()
    # the claims of the failed call are gone: a call without a reset starts from an empty map
    k, n_kept = ctx.dedup_device(c2.dev, reset=False)
    assert np.array_equal(k.numpy(np.uint8), c2.dedup) and n_kept == int(c2.dedup.sum())
    # the argument errors that need a context
    assert L.eg3d_dedup_device(ctx._h, None, 0, 1, keep.ptr, None) == -1
    assert L.eg3d_dedup_device(ctx._h, C.byref(c2.dev), 0, 1, None, None) == -1
    assert L.eg3d_dedup_device(ctx._h, C.byref(c2.dev), 2**32 - 1 - c2.n, 1, keep.ptr, None) == -1
    assert b"index_base" in L.eg3d_last_error()
    part = c2.view(c2.n)
    part.complete = 0
    assert L.eg3d_dedup_device(ctx._h, C.byref(part), 0, 1, keep.ptr, None) == -1
    # the largest index_base that fits
    k, n_kept = ctx.dedup_device(c2.dev, index_base=2**32 - 2 - c2.n, reset=True)
    assert np.array_equal(k.numpy(np.uint8), c2.dedup)


@pytest.mark.parametrize("to_host", [True, False], ids=["to host", "device only"])
def test_dedup_resident_without_the_filter(c2, to_host):
    want = np_compact(c2.cloud, c2.dedup)
    got, dev, st = c2.ctx.dedup_resident(to_host=to_host)
    print("dedup_resident: %d -> %d; dedup %.3f ms, compact %.3f ms, copy %.3f ms"
          % (st["n_points_in"], st["n_kept"], st["ms_dedup"], st["ms_compact"], st["ms_copy"]))
    assert same_cloud(c2.ctx.fetch_device_points(dev, 0, int(dev.n_points)), want) is None
    if to_host:
        assert same_cloud(got, want) is None and int(got["obs_off"][-1]) == want["n_obs"]
    else:
        assert got is None and st["ms_copy"] == 0
    assert st["struct_size"] == C.sizeof(D.DedupStats) and st["threshold"] == -1
    assert st["n_points_in"] == c2.n and st["n_dedup_kept"] == st["n_kept"] == want["n_points"] == int(c2.dedup.sum())
    assert st["n_obs_kept"] == want["n_obs"] and st["n_gn_inliers"] == 0 and 0 < st["n_kept"] < c2.n
    assert st["ms_dedup"] > 0 and st["ms_compact"] > 0 and st["ms_filter"] == 0


@pytest.mark.parametrize("forced", [-1, 4])
@pytest.mark.parametrize("with_base", [False, True], ids=["no base_hist", "base_hist"])
def test_dedup_resident_with_the_filter(c2, with_base, forced):
    """The sequence of test_reference_order_dedup_mask_then_filter: host dedup, oracle filter on the deduplicated cloud,
    host threshold, numpy compaction."""
    small = np_compact(c2.cloud, c2.dedup)
    Xs, inls = c2.oracle_filter(small, c2.mse)
    sfm_k = np.random.default_rng(9).integers(2, c2.V + 1, 50000).astype(np.int64) if with_base else None
    thr, surv = host_threshold(c2.V, np.diff(small["obs_off"].astype(np.int64)), inls, forced, sfm_k)
    want = np_compact(small, surv, Xs)
    base = np.bincount(sfm_k, minlength=c2.V + 1).astype(np.uint64) if with_base else None
    got, dev, st = c2.ctx.dedup_resident(with_filter=True, gn_max_mse=c2.mse, forced_min_filter=forced, base_hist=base)
    print("dedup_resident + filter: threshold %d, %d -> %d -> %d inliers -> %d; dedup %.3f, filter %.3f, compact %.3f, copy %.3f ms"
          % (st["threshold"], st["n_points_in"], st["n_dedup_kept"], st["n_gn_inliers"], st["n_kept"], st["ms_dedup"],
             st["ms_filter"], st["ms_compact"], st["ms_copy"]))
    assert st["threshold"] == thr
    assert st["n_points_in"] == c2.n and st["n_dedup_kept"] == small["n_points"] and st["n_gn_inliers"] == int(inls.sum())
    assert st["n_kept"] == want["n_points"] and st["n_obs_kept"] == want["n_obs"]
    assert 0 < want["n_points"] < small["n_points"]
    assert same_cloud(got, want) is None
    assert same_cloud(c2.ctx.fetch_device_points(dev, 0, int(dev.n_points)), want) is None


def test_a_clone_has_claims_of_its_own(c2):
    half = c2.n // 2
    clone = c2.ctx.clone()
    try:
        c2.ctx.dedup_device(c2.view(half), 0, True)                  # the parent claims the first half's cells
        second = D.DeviceEdgePoints()
        C.memmove(C.byref(second), C.byref(c2.dev), C.sizeof(second))
        # the second half as a view of its own: the same observation arrays, the offsets from point `half` on (the
        # observations in front of the first list belong to no point)
        second.n_points = c2.n - half
        tail = c2.ctx.upload(c2.cloud["obs_off"][half:-1])
        second.obs_off = tail.ptr
        alone = dc.host_mask(dc.slice_cloud(c2.cloud, half, c2.n), c2.V, c2.W, c2.H)
        kc, _ = clone.dedup_device(second, half, False)              # the clone has seen nothing: the part alone
        assert np.array_equal(kc.numpy(np.uint8), alone)
        kp, _ = c2.ctx.dedup_device(second, half, False)             # the parent continues its own claims
        assert np.array_equal(kp.numpy(np.uint8), c2.dedup[half:])
        assert not np.array_equal(alone, c2.dedup[half:])
        kp2, _ = c2.ctx.dedup_device(c2.view(half), 0, False)        # ... and the clone's claims did not reach its map
        assert np.array_equal(kp2.numpy(np.uint8)[:half], c2.dedup[:half])
    finally:
        clone.close()
