"""The 3 px dedup as an order-independent rule, pinned on the CPU before any kernel: cloudnp.np_dedup (a minimum per
cell, one test per point) == eg3d_host_filter_close_2d (the sequential host step) == orc_filter_close_2d (the oracle),
byte for byte, on the oracle's clouds of synthetic configs 1 and 2 and on hand-built hostile clouds; and the
concatenation property that dedup across calls rests on."""
import ctypes as C

import numpy as np
import pytest

import dedup_cases as dc
from edgegraph3d_amd import host
from edgegraph3d_amd.cloudnp import dedup_claims, np_dedup
from oracle import binding as ob

_SYNTH = {}


def _synth_cloud(cfg):
    if cfg not in _SYNTH:
        s = host.Synth(cfg)
        o = ob.Oracle(s.scene)
        _SYNTH[cfg] = (s, o, o.match(s.seeds, 0, int(s.seeds.contents.n_seeds), 16))
    return _SYNTH[cfg]


def _check_concatenation(cloud, V, W, H, whole, cuts):
    n = int(cloud["n_points"])
    for cut in cuts:
        a, b = dc.slice_cloud(cloud, 0, cut), dc.slice_cloud(cloud, cut, n)
        claims = dedup_claims(V, W, H)
        ka = np_dedup(a, V, W, H, claims, 0)
        kb = np_dedup(b, V, W, H, claims, cut)
        assert np.array_equal(np.concatenate([ka, kb]), whole), cut
        assert np.array_equal(ka, dc.host_mask(a, V, W, H)), cut   # the mask of a prefix is the prefix of the mask


@pytest.mark.parametrize("cfg,kept,total", [(1, 4356, 8247), (2, 58676, 209531)])
def test_rule_on_the_oracle_clouds(cfg, kept, total):
    s, o, cloud = _synth_cloud(cfg)
    sc = s.scene.contents
    V, W, H = int(sc.n_views), int(sc.width), int(sc.height)
    kh, ko, kn = dc.host_mask(cloud, V, W, H), dc.oracle_mask(o, cloud), np_dedup(cloud, V, W, H)
    print("Synth(%d): %d of %d kept" % (cfg, kh.sum(), len(kh)))
    assert len(kh) == total and int(kh.sum()) == kept
    assert kh.any() and not kh.all(), "both verdicts must occur"
    assert np.array_equal(kn, kh) and np.array_equal(ko, kh)
    n = len(kh)
    _check_concatenation(cloud, V, W, H, kh, (1, n // 3, n // 2 + 7, n - 1))
    # three parts, as the reference's three pipeline stages
    claims, parts, base = dedup_claims(V, W, H), [], 0
    for p0, p1 in ((0, n // 4), (n // 4, n // 4), (n // 4, 2 * n // 3), (2 * n // 3, n)):
        parts.append(np_dedup(dc.slice_cloud(cloud, p0, p1), V, W, H, claims, base))
        base += p1 - p0
    assert np.array_equal(np.concatenate(parts), kh)


@pytest.mark.parametrize("name", list(dc.hostile_clouds()))
def test_rule_on_hostile_clouds(name):
    V, W, H = dc.HOSTILE_RIG
    assert W % 3 and H % 3
    cloud, trivial = dc.hostile_clouds()[name]
    s = host.Synth(1)
    assert int(s.scene.contents.n_views) == V
    sc = dc.scene_with_size(s.scene, W, H)
    o = ob.Oracle(C.byref(sc))
    kh, ko, kn = dc.host_mask(cloud, V, W, H), dc.oracle_mask(o, cloud), np_dedup(cloud, V, W, H)
    print("%s: %d of %d kept" % (name, kh.sum(), len(kh)))
    if trivial:
        assert not kh.any()
    else:
        assert kh.any() and not kh.all(), "both verdicts must occur"
    assert np.array_equal(kn, kh) and np.array_equal(ko, kh)
    n = len(kh)
    _check_concatenation(cloud, V, W, H, kh, sorted({0, 1, n // 2, n - 1, n}))


def test_hostile_clouds_hold_what_they_claim():
    V, W, H = dc.HOSTILE_RIG
    clouds = dc.hostile_clouds()
    xy = np.concatenate([c["obs_xy"] for c, _ in clouds.values()])
    view = np.concatenate([c["obs_view"] for c, _ in clouds.values()])
    assert np.isnan(xy).any() and np.isposinf(xy).any() and np.isneginf(xy).any()
    assert ((xy > -3) & (xy < 0)).any() and (xy[:, 0] == W).any() and (xy[:, 1] == H).any()
    assert (xy[:, 0] > W).any() and (xy[:, 1] > H).any()
    assert (view == -1).any() and (view == V).any()
    k = np.diff(clouds["mixed large"][0]["obs_off"].astype(np.int64))
    assert (k == 0).sum() > 300 and k.max() >= 9
    one = clouds["one cell"][0]
    assert len(set(map(tuple, np.trunc(one["obs_xy"] / np.float32(3)).astype(int)))) == 1


def test_index_range():
    V, W, H = dc.HOSTILE_RIG
    cloud = dc.make_cloud([[(0, 1.0, 1.0)]])
    with pytest.raises(ValueError):
        np_dedup(cloud, V, W, H, None, 2**32 - 2)
    assert np_dedup(cloud, V, W, H, None, 2**32 - 3).tolist() == [1]
