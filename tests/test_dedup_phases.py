"""The 3 px dedup in phases, pinned on the CPU (include/eg3d_host_dedup_phases.h, cloudnp.np_claim / np_keep): clouds cut
into parts BETWEEN POINTS, the parts claimed in any order — into one map, or into one map per part joined by the merge —
and then kept part by part give, concatenated, the mask of the sequential dedup of the whole cloud
(eg3d_host_filter_close_2d == orc_filter_close_2d == np_dedup), byte for byte. Hand-made hostile clouds and the oracle's
C2 cloud; the cuttings into 3 and 7 parts have an empty part. And the two conditions without which these tests would prove
nothing: a part deduplicated alone keeps MORE than its share, and the combined claim-and-keep rule applied part by part in
reversed order gives ANOTHER mask."""
import ctypes as C

import numpy as np
import pytest

import dedup_cases as dc
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import host
from edgegraph3d_amd.cloudnp import dedup_claims, np_claim, np_dedup, np_keep
from test_dedup_rule import _synth_cloud

UNCLAIMED = 0xFFFFFFFF


def cuttings(n):
    """{parts: bounds}: 1, 2, 3 and 7 parts of n points; the cuts fall anywhere (no regard for chains), and the cuttings
    into 3 and 7 parts have an empty part."""
    return {1: [0, n], 2: [0, n // 3 + 1, n], 3: [0, n // 4 + 1, n // 4 + 1, n],
            7: [0, n // 9, n // 5 + 1, n // 3, n // 3, n // 2 + 3, min(n, 4 * n // 5 + 2), n]}


def orders(k):
    fixed = list(np.random.default_rng(20261020).permutation(k))
    return {"forward": list(range(k)), "reversed": list(range(k))[::-1], "shuffled": [int(i) for i in fixed]}


def phased_masks(cloud, V, W, H, bounds, order, per_part_maps, use_numpy):
    """The concatenated keep masks of the parts, and the final map."""
    bounds = [min(max(b, 0), int(cloud["n_points"])) for b in bounds]
    bounds = [max(b, a) for a, b in zip([0] + bounds[:-1], bounds)]
    parts = [dc.slice_cloud(cloud, a, b) for a, b in zip(bounds[:-1], bounds[1:])]
    empty = (lambda: dedup_claims(V, W, H)) if use_numpy else (lambda: host.dedup_empty_claims(V, W, H))
    claim = (lambda p, m, base: np_claim(p, m, base)) if use_numpy else (lambda p, m, base: host.dedup_claim(p, V, W, H, m, base))
    first = empty()
    for i in order:
        if per_part_maps:
            mine = claim(parts[i], empty(), bounds[i])
            if use_numpy:
                np.minimum(first, mine, out=first)
            else:
                host.dedup_merge(first, mine)
        else:
            claim(parts[i], first, bounds[i])
    masks = []
    for i in reversed(range(len(parts))):   # (the keep passes in any order too: they only read the map)
        if use_numpy:
            masks.append(np_keep(parts[i], first, bounds[i]))
        else:
            m, n_kept = host.dedup_keep(parts[i], V, W, H, first, bounds[i])
            assert n_kept == int(m.sum())
            masks.append(m)
    return np.concatenate(masks[::-1]), first


def check_all_orders(cloud, V, W, H, want, statements=(False, True)):
    n = int(cloud["n_points"])
    maps = []
    for k, bounds in cuttings(n).items():
        for oname, order in orders(len(bounds) - 1).items():
            for per_part in (False, True):
                for use_numpy in statements:
                    got, first = phased_masks(cloud, V, W, H, bounds, order, per_part, use_numpy)
                    assert np.array_equal(got, want), (k, oname, per_part, use_numpy)
                    maps.append(np.asarray(first).reshape(-1))
    for m in maps[1:]:   # one cloud, one map, whatever the route
        assert np.array_equal(m, maps[0])


@pytest.mark.parametrize("name", list(dc.hostile_clouds()))
def test_phases_on_hostile_clouds(name):
    V, W, H = dc.HOSTILE_RIG
    cloud, trivial = dc.hostile_clouds()[name]
    s = host.Synth(1)
    sc = dc.scene_with_size(s.scene, W, H)
    from oracle import binding as ob
    want = dc.host_mask(cloud, V, W, H)
    assert np.array_equal(want, dc.oracle_mask(ob.Oracle(C.byref(sc)), cloud)) and np.array_equal(want, np_dedup(cloud, V, W, H))
    assert trivial or (want.any() and not want.all())
    check_all_orders(cloud, V, W, H, want)


def _c2():
    s, o, cloud = _synth_cloud(2)
    sc = s.scene.contents
    return s, o, cloud, int(sc.n_views), int(sc.width), int(sc.height)


def test_phases_on_the_c2_cloud():
    s, o, cloud, V, W, H = _c2()
    want = dc.host_mask(cloud, V, W, H)
    assert np.array_equal(want, dc.oracle_mask(o, cloud)) and np.array_equal(want, np_dedup(cloud, V, W, H))
    assert want.any() and not want.all()
    # some cut of every cutting with parts falls INSIDE a chain (equal key[0..2] on both sides): points, not chains, are cut
    key, n = cloud["key"], int(cloud["n_points"])
    for k, bounds in cuttings(n).items():
        if k > 1:
            assert any(0 < b < n and np.array_equal(key[b - 1][:3], key[b][:3]) for b in bounds), k
    # (the host statement on every route; the numpy statement on the two routes of the 7-part cutting below)
    check_all_orders(cloud, V, W, H, want, statements=(False,))
    for per_part in (False, True):
        got, _ = phased_masks(cloud, V, W, H, cuttings(n)[7], orders(7)["shuffled"], per_part, True)
        assert np.array_equal(got, want)


def test_conditions_that_keep_these_tests_honest():
    s, o, cloud, V, W, H = _c2()
    n = int(cloud["n_points"])
    want = dc.host_mask(cloud, V, W, H)
    thirds = [0, n // 3, 2 * n // 3, n]
    parts = [dc.slice_cloud(cloud, a, b) for a, b in zip(thirds[:-1], thirds[1:])]
    # (1) the last third deduplicated alone keeps MORE points than its share of the global mask: earlier parts own cells
    alone = dc.host_mask(parts[2], V, W, H)
    print("last third: %d kept alone, %d within the whole cloud" % (alone.sum(), want[thirds[2]:].sum()))
    assert alone.sum() > want[thirds[2]:].sum()
    # (2) the combined rule (claim and keep back to back, as eg3d_dedup_device) applied part by part in REVERSED order,
    # with the right global bases, does not give the global mask: a keep pass ran before an earlier part had claimed
    claims, masks = dedup_claims(V, W, H), [None] * 3
    for i in (2, 1, 0):
        masks[i] = np_dedup(parts[i], V, W, H, claims, thirds[i])
    rev = np.concatenate(masks)
    print("combined rule in reversed order: %d kept, the whole cloud %d" % (rev.sum(), want.sum()))
    assert not np.array_equal(rev, want) and rev.sum() > want.sum()
    # ... while the phases in that order do
    got, _ = phased_masks(cloud, V, W, H, thirds, [2, 1, 0], False, False)
    assert np.array_equal(got, want)


def test_host_refusals_leave_the_map_as_it_was():
    V, W, H = dc.HOSTILE_RIG
    L = host.lib()
    cloud = dc.hostile_clouds()["mixed small"][0]
    n = int(cloud["n_points"])
    first = host.dedup_empty_claims(V, W, H)
    assert first.size == L.eg3d_host_dedup_n_cells(V, W, H) == V * 533 * 400 and (first == UNCLAIMED).all()
    host.dedup_claim(dc.slice_cloud(cloud, 0, n // 2), V, W, H, first, 0)
    before = first.copy()
    assert (before != UNCLAIMED).any()
    # offsets that do not ascend ...
    bad = dict(cloud)
    bad["obs_off"] = cloud["obs_off"].copy()
    bad["obs_off"][n // 3] = bad["obs_off"][n // 3 + 1] + 5
    with pytest.raises(ValueError):
        host.dedup_claim(bad, V, W, H, first, 0)
    with pytest.raises(ValueError):
        host.dedup_keep(bad, V, W, H, first, 0)
    assert np.array_equal(first, before)
    # ... and a last list that ends beyond n_obs
    short, keep = D.EdgePointsArrays(cloud), np.zeros(n, np.uint8)
    short.c.n_obs = int(cloud["n_obs"]) - 1
    assert L.eg3d_host_dedup_claim(V, W, H, C.byref(short.c), 0, D.np_ptr(first, C.c_uint32)) == -1
    assert L.eg3d_host_dedup_keep(V, W, H, C.byref(short.c), 0, D.np_ptr(first, C.c_uint32), D.np_ptr(keep, C.c_uint8), None) == -1
    assert np.array_equal(first, before) and not keep.any()
    # the index range: index_base + n_points stays below 2^32 - 1
    with pytest.raises(ValueError):
        host.dedup_claim(cloud, V, W, H, first, 2**32 - 1 - n)
    assert np.array_equal(first, before)
    ep, one = D.EdgePointsArrays(cloud), np.zeros(1, np.uint32)
    assert L.eg3d_host_dedup_claim(0, W, H, C.byref(ep.c), 0, D.np_ptr(first, C.c_uint32)) == -1
    assert L.eg3d_host_dedup_claim(V, W, H, None, 0, D.np_ptr(first, C.c_uint32)) == -1
    assert L.eg3d_host_dedup_claim(V, W, H, C.byref(ep.c), 0, None) == -1
    assert L.eg3d_host_dedup_merge(None, D.np_ptr(one, C.c_uint32), 1) == -1
    assert np.array_equal(first, before)
    # the largest base that fits claims with it
    top = host.dedup_empty_claims(V, W, H)
    host.dedup_claim(cloud, V, W, H, top, 2**32 - 2 - n)
    m, _ = host.dedup_keep(cloud, V, W, H, top, 2**32 - 2 - n)
    assert np.array_equal(m, dc.host_mask(cloud, V, W, H)) and int(top.min()) >= 2**32 - 2 - n
    # the rest of the run continues from the map that survived the refusals
    host.dedup_claim(dc.slice_cloud(cloud, n // 2, n), V, W, H, first, n // 2)
    m, _ = host.dedup_keep(cloud, V, W, H, first, 0)
    assert np.array_equal(m, dc.host_mask(cloud, V, W, H))


def test_merge_is_the_elementwise_minimum():
    rng = np.random.default_rng(3)
    for n in (0, 1, 5, 1000):
        a = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        b = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        b[::3] = a[::3]
        a[1::7] = UNCLAIMED
        want = np.minimum(a, b)
        got = a.copy()
        if n:
            host.dedup_merge(got, b)
        assert np.array_equal(got, want)
