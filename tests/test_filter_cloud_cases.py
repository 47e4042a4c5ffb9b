"""The hand-built clouds of tests/filter_cloud_cases.py reach what they are for — checked with the CPU oracle alone, so
that the GPU tests on them (tests/test_gpu_filter_device_paths.py) cannot pass vacuously: both verdicts at every listed
list length, accepted points that moved, staged and unstaged blocks, inliers in the overflow bin, and for threshold16 an
observation threshold that the overflow rule decides."""
import ctypes as C

import numpy as np
import pytest

import filter_cloud_cases as fc
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import host
from edgegraph3d_amd.cloudnp import np_compact


@pytest.mark.parametrize("legacy", [False, True], ids=["abs", "legacy abs"])
@pytest.mark.parametrize("name", fc.K5_CASES)
def test_case_reaches_its_paths(name, legacy):
    c = fc.case(name)
    Xr, ir = c.oracle(legacy)
    inl = ir != 0
    print(c.coverage(ir))
    for k in fc.LISTED_LENGTHS[name]:
        assert (c.k == k).sum() >= 4, k
    for k in c.both_verdicts:
        assert inl[c.k == k].any() and not inl[c.k == k].all(), (k, "both verdicts")
    for k in set(fc.LISTED_LENGTHS[name]) - set(c.both_verdicts):
        # fewer than two observations: the normal matrix is singular and the oracle rejects the point (one verdict only).
        # Under the legacy abs() a pass whose mse is below 1 counts as converged before any solve, so a single observation
        # that starts that close is accepted where it stands; an empty list (mse 0 / 0) never is.
        if k == 0 or (k == 1 and not legacy):
            assert not inl[c.k == k].any(), k
    moved = (Xr.view(np.uint32) != c.X.view(np.uint32)).any(axis=1)
    assert (moved & inl).any(), "some accepted point must have moved"
    assert not (moved & ~inl).any(), "a rejected point keeps its position"
    # light and heavy blocks, and what the kernel makes of them on this rig
    assert (c.per_block <= fc.K5_OBS_CAP).any() and (c.per_block > fc.K5_OBS_CAP).any()
    if c.V <= fc.K5_VIEW_CAP:
        assert c.staged.any() and not c.staged.all()
        # ... and the decision changes from one block of the launch to the next
        assert (np.diff(c.staged.astype(np.int8)) != 0).any()
    else:
        assert not c.staged.any()
    over = c.k > c.V
    assert int((inl & over).sum()) >= 4, "inliers of the overflow bin"
    for k in np.unique(c.k[over]):
        if k in fc.LISTED_LENGTHS[name]:
            assert int((inl & (c.k == k)).sum()) >= 4, (k, "inliers of the overflow bin at this length")
    # every bucket of the counting sort: empty lists (where the case has them), 1 .. 63, the shared bucket of 64 or more
    assert (c.k >= 64).sum() >= 4 or name == "threshold16"


def test_rig16_shape():
    c = fc.case("rig16")
    assert c.n % 256 and c.n % 64 and len(c.per_block) == 4
    assert list(c.heavy) == [False, True, False, False] and list(c.staged) == [True, False, True, True]
    assert (c.k == 0).sum() >= 4 and (c.k > c.V).any()
    assert len(c.off) == c.n + 1 and int(c.off[-1]) == len(c.view) == len(c.xy)


@pytest.mark.parametrize("V", [256, 257])
def test_wide_rig_shapes(V):
    c = fc.case("rig%d" % V)
    assert c.V == V and list(c.heavy) == [False, True]
    assert list(c.staged) == ([True, False] if V == 256 else [False, False])
    assert (c.k == V + 1).sum() >= 4 and (c.k == 258).sum() >= 4      # 258 lands in the overflow bin of both rigs
    assert c.view.min() == 0 and c.view.max() == V - 1


def _threshold(hist, V, count):
    """The median loop of eg3d_host_observation_filter on hist[k], k = 0 .. V, with `count` points in all."""
    acc, median = 0, V
    for m in range(V):
        acc += int(hist[m + 1])
        if acc >= count // 2:
            median = m
            break
    return max(3, median // 2 - 1)


def test_threshold16_is_decided_by_the_overflow_rule():
    from edgegraph3d_amd.distributed import observation_threshold
    c = fc.case("threshold16")
    _, ir = c.oracle(False)
    inl = ir != 0
    V = c.V
    thr, surv = fc.host_threshold(V, c.k, ir)
    fits = inl & (c.k <= V)
    hist = np.bincount(c.k[fits], minlength=V + 1)
    right = _threshold(hist, V, int(inl.sum()))                     # counted, in no bin
    binned_at_V = hist.copy()
    binned_at_V[V] += int((inl & (c.k > V)).sum())
    wrong_bin = _threshold(binned_at_V, V, int(inl.sum()))          # wrong: over-long lists binned at V
    wrong_count = _threshold(hist, V, int(fits.sum()))              # wrong: over-long lists left out of the count
    print("%s; thresholds: host %d, numpy %d, binned at V %d, left out of the count %d; hist %s"
          % (c.coverage(ir), thr, right, wrong_bin, wrong_count, hist.tolist()))
    assert thr == right == observation_threshold(hist, V, -1, count=int(inl.sum()))
    assert len({thr, wrong_bin, wrong_count}) > 1, "the three rules must not all agree"
    assert thr != wrong_bin and thr != wrong_count
    assert thr > 3
    # the threshold separates survivors: some inliers fall at or below it, some lie above
    assert 0 < surv.sum() < inl.sum()
    assert np.array_equal(surv != 0, inl & (c.k > thr))


@pytest.mark.parametrize("name", ["rig16", "rig257"])
def test_masks(name):
    c = fc.case(name)
    _, ir = c.oracle(False)
    inl = ir != 0
    seen = set()
    for mn in fc.MASKS:
        m = fc.mask(c, mn)
        assert m.dtype == np.uint8 and len(m) == c.n
        seen.add(m.tobytes())
        if mn not in ("ones", "zeros"):
            assert (inl & (m != 0)).any() and (inl & (m == 0)).any(), mn     # the mask changes the inlier set
    assert len(seen) == len(fc.MASKS)
    b, h = c.first_light(), c.first_heavy()
    assert not fc.mask(c, "block_off")[b * 256:(b + 1) * 256].any() and fc.mask(c, "block_off").sum() == c.n - 256
    w = fc.mask(c, "wave_off")
    assert not w[h * 256 + 64:h * 256 + 128].any() and w.sum() == c.n - 64
    r = fc.mask(c, "random50")
    assert 0.4 < r.mean() < 0.6


def test_lone_empty_list_between_two_long_ones():
    c = fc.case("rig16")
    m = fc.lone_empty_between_long(c)
    i = np.flatnonzero(m)
    assert len(i) == 3 and i[0] // 64 == i[2] // 64 and c.heavy[i[0] // 256]
    assert c.k[i[0]] >= 64 and c.k[i[1]] == 0 and c.k[i[2]] >= 64
    cloud = fc.host_cloud(c.X, c.off, c.view, c.xy)
    out = np_compact(cloud, m)
    assert out["n_points"] == 3 and out["obs_off"][1] == out["obs_off"][2] == c.k[i[0]]
    assert fc.lone_empty_between_long(fc.case("rig257")) is None     # (no empty lists there)


def test_host_cloud_layout():
    c = fc.case("rig16")
    cloud = fc.host_cloud(c.X, c.off, c.view, c.xy)
    assert cloud["obs_off"].dtype == np.uint64 and len(cloud["obs_off"]) == c.n + 1 and cloud["obs_off"][-1] == c.n_obs
    for name in ("obs_pl", "obs_seg"):
        assert len(np.unique(cloud[name])) == c.n_obs
    assert len(np.unique(cloud["key"])) == 4 * c.n
    everything = np_compact(cloud, np.ones(c.n, np.uint8))
    assert everything["n_points"] == c.n and np.array_equal(everything["obs_off"], cloud["obs_off"])


def test_dedup_reference_on_rig16_is_not_trivial():
    """What the GPU dedup test compares with: eg3d_host_filter_close_2d on the rig16 cloud drops every empty list and at
    least one point that has observations, and keeps points with lists longer than the 8 lanes a point gets."""
    c = fc.case("rig16")
    sc = c.s.scene.contents
    ep = D.EdgePointsArrays(fc.host_cloud(c.X, c.off, c.view, c.xy))
    keep = np.zeros(c.n, np.uint8)
    assert host.lib().eg3d_host_filter_close_2d(c.V, int(sc.width), int(sc.height), C.byref(ep.c), D.np_ptr(keep, C.c_uint8)) == 0
    print("rig16 dedup: kept %d of %d; dropped with observations %d; kept with more than 8 observations %d"
          % (keep.sum(), c.n, ((keep == 0) & (c.k > 0)).sum(), ((keep != 0) & (c.k > 8)).sum()))
    assert not keep[c.k == 0].any()
    assert ((keep == 0) & (c.k > 0)).any() and ((keep != 0) & (c.k > 8)).sum() >= 4


@pytest.mark.parametrize("n", [fc.K6_SCAN_TRIP, fc.K6_SCAN_TRIP + 3 * 256 + 5])
def test_scan_cloud(n):
    X, off, view, xy = fc.scan_cloud(n)
    assert len(X) == n and len(off) == n + 1 and int(off[-1]) == len(view) == len(xy)
    assert set(np.diff(off.astype(np.int64)).tolist()) == {0, 1, 2, 3}
    assert (n + 255) // 256 > 1024 or n == 1024 * 256      # exactly one trip of the scan, or a second one
