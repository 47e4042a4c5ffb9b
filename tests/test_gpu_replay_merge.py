"""-m gpu: the matches manager merges the GRAPHS of later shards on the device (eg3d_replay_merge_graph, K8m). Every shard is
replayed on a clone (eg3d_replay_device) and its graph merged into another context's accumulator; every graph is compared
field for field and bit for bit (replay_gpu_cases.same_graph) with the oracle's replay of the concatenation of the shards'
clouds, and with eg3d_replay_device on the one-call cloud. The reference is never the merge itself."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import replay_gpu_cases as rc
import replay_merge_cases as mc
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host
from oracle import binding as ob
from test_replay_accumulate import chain_starts, concat, parts_at, slice_cloud, _ranges

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _live():
    f = api.lib().eg3d_test_live_device_bytes
    f.restype, f.argtypes = C.c_int64, []
    return int(f())


@pytest.fixture(scope="module")
def small():
    sa = rc.small_scene()
    return sa, ob.Oracle(C.byref(sa.c)), rc.cases()


def _n_pairs(cloud):
    return cloud["n_points"] - 1 - len(chain_starts(cloud)) if cloud["n_points"] else 0


def _check_step(ctx, got, dv, st, want, pairs, points, what):
    assert rc.same_graph(got, want) is None, (what, rc.same_graph(got, want))
    back = ctx.fetch_device_graph(dv)
    assert rc.same_graph(back, got) is None, (what, "device view", rc.same_graph(back, got))
    assert st["struct_size"] == C.sizeof(D.ReplayStats)
    assert (st["n_pairs"], st["n_nodes"], st["n_polylines"], st["n_intervals"]) == \
        (pairs, want["n_nodes"], want["n_polylines"], int(want["iv_off"][-1])), (what, st)
    tot = ctx.replay_accumulated()
    assert (tot["n_points"], tot["n_pairs"]) == (points, pairs), (what, tot)


class Pool:
    """A context and the clones handed out from it, at most `cap` at a time."""

    def __init__(self, scene, cap):
        self.first, self.cap = api.Context(scene), cap
        self.free, self.all = [self.first], [self.first]

    def take(self):
        if not self.free:
            assert len(self.all) < self.cap
            self.all.append(self.first.clone())
            self.free.append(self.all[-1])
        return self.free.pop()

    def give(self, ctx):
        self.free.append(ctx)

    def close(self):
        for c in reversed(self.all):
            c.close()


def _replayed(ctx, part):
    """The part's graph on `ctx`, by eg3d_replay_device: (DeviceGraph3D, points, pairs, what keeps the upload alive)."""
    d, held = rc.upload_cloud(ctx, part)
    _, dv, st = ctx.replay_device(d, to_host=False)
    assert st["n_pairs"] == _n_pairs(part)
    return dv, part["n_points"], st["n_pairs"], held


def _tree(pool, parts, lo, hi, check):
    """Pairwise tree over parts[lo:hi]: (DeviceGraph3D, points, pairs, the context whose buffers it views)."""
    if hi - lo == 1:
        ctx = pool.take()
        dv, n, pr, _ = _replayed(ctx, parts[lo])
        return dv, n, pr, ctx
    mid = (lo + hi) // 2
    left = _tree(pool, parts, lo, mid, check)
    right = _tree(pool, parts, mid, hi, check)
    acc = pool.take()
    got, dv, st = acc.replay_merge(left[0], left[1], left[2], reset=True)
    check(acc, got, dv, st, lo, mid)
    got, dv, st = acc.replay_merge(right[0], right[1], right[2])
    check(acc, got, dv, st, lo, hi)
    pool.give(left[3]), pool.give(right[3])
    return dv, left[1] + right[1], left[2] + right[2], acc


# ---- 1. hand-built clouds, every subset of their chain boundaries, fold and tree -------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_every_cut_of_a_hand_built_cloud(eg3d_form, small, name):
    sa, o, clouds = small
    cloud = clouds[name]
    starts = chain_starts(cloud)
    pool = Pool(C.byref(sa.c), 5)
    try:
        acc, worker = pool.take(), pool.take()
        for r in range(len(starts) + 1):
            for cuts in itertools.combinations(starts, r):
                parts = parts_at(cloud, cuts)
                if len(parts) > 1:
                    parts = parts[:1] + [slice_cloud(cloud, 0, 0)] + parts[1:]      # an empty part in the middle changes nothing
                wants = {}

                def check(ctx, got, dv, st, lo, hi):
                    if (lo, hi) not in wants:
                        wants[(lo, hi)] = concat(parts[lo:hi])
                        wants[(lo, hi)] = (o.replay_matches(wants[(lo, hi)]), _n_pairs(wants[(lo, hi)]), wants[(lo, hi)]["n_points"])
                    want, pairs, points = wants[(lo, hi)]
                    _check_step(ctx, got, dv, st, want, pairs, points, (name, cuts, lo, hi))

                for i, p in enumerate(parts):      # the fold: every part replayed on the clone, merged into the first context
                    dvp, n, pr, held = _replayed(worker, p)
                    got, dv, st = acc.replay_merge(dvp, n, pr, reset=(i == 0))
                    check(acc, got, dv, st, 0, i + 1)
                assert rc.same_graph(got, o.replay_matches(cloud)) is None, (name, cuts)
        # ... and once as a pairwise tree, at the finest cut
        pool.give(acc), pool.give(worker)
        parts = parts_at(cloud, starts)
        wants = {}
        dv, n, pr, ctx = _tree(pool, parts, 0, len(parts), check)
        assert n == cloud["n_points"] and pr == _n_pairs(cloud)
        assert rc.same_graph(ctx.fetch_device_graph(dv), o.replay_matches(cloud)) is None, (name, "tree")
        assert 2 <= len(pool.all) <= 5
    finally:
        pool.close()


# ---- 2. matched clouds, one clone per seed range ------------------------------------------------------------------------------------
_CACHE = {}


class Shards:
    """Per DLT form: synthetic config 0 (whole) and the C2 window of tests/test_gpu_replay_device.py, each with a context
    whose seeds are resident, five clones, the one-call cloud, the oracle's graph of it and eg3d_replay_device's."""

    def __init__(self):
        self.items = {}
        for name, cfg, window in (("config0", 0, None), ("c2_window", 2, (1550, 1800))):
            s = host.Synth(cfg)
            ctx = api.Context(s.scene)
            ctx.upload_seeds(s.seeds)
            b, e = (0, s.n_seeds) if window is None else window
            ctx.match_resident(b, e, device_only=True)
            cloud = ctx.fetch_device_output()
            one_shot, _, st = ctx.replay_device()
            clones = [ctx.clone() for _ in range(5)]
            self.items[name] = (s, ctx, clones, (b, e), cloud, ob.Oracle(s.scene).replay_matches(cloud), one_shot, st)

    def close(self):
        for s, ctx, clones, *_ in self.items.values():
            for c in clones:
                c.close()
            ctx.close()


def _drop_cache():
    import forms
    for rows, m in list(_CACHE.items()):
        with forms.product_form(rows):
            m.close()
    _CACHE.clear()


@pytest.fixture
def shards(eg3d_form):
    if eg3d_form not in _CACHE:
        _drop_cache()
        _CACHE[eg3d_form] = Shards()
    return _CACHE[eg3d_form]


@pytest.fixture(scope="module", autouse=True)
def _close_cached_contexts():
    yield
    _drop_cache()


def _shard_graph(clone, rb, re):
    d = clone.match_resident(rb, re, device_only=True)
    _, dv, st = clone.replay_device(to_host=False)
    return dv, d["n_points"], st["n_pairs"]


@pytest.mark.parametrize("name", ["config0", "c2_window"])
def test_shards_replayed_on_clones_fold_to_the_one_call_graph(shards, name):
    s, ctx, clones, (b, e), cloud, want, one_shot, st1 = shards.items[name]
    assert rc.same_graph(one_shot, want) is None
    for k in (2, 3, 5):
        graphs = [_shard_graph(clones[i], rb, re) for i, (rb, re) in enumerate(_ranges(b, e, k))]
        assert sum(g[1] for g in graphs) == cloud["n_points"]
        for i, (dv, n, pr) in enumerate(graphs):
            got, dva, st = ctx.replay_merge(dv, n, pr, reset=(i == 0), materialise=(i == k - 1))
        _check_step(ctx, got, dva, st, want, st1["n_pairs"], cloud["n_points"], (name, k))
        assert rc.same_graph(got, one_shot) is None, (name, k, rc.same_graph(got, one_shot))
        if name == "c2_window":      # the condition: the shards' graphs hold more than the whole; concatenating them would not pass
            nodes = sum(int(g[0].n_nodes) for g in graphs)
            pls = sum(int(g[0].n_polylines) for g in graphs)
            assert nodes > want["n_nodes"] and pls > want["n_polylines"], (nodes, pls)


# ---- 3. clouds and graphs mixed; the extractor reads the merged intervals in place -----------------------------------------------
def test_a_mixture_of_clouds_and_graphs_and_the_extractor(shards):
    s, ctx, clones, (b, e), cloud, want, one_shot, st1 = shards.items["c2_window"]
    n_sets, row_off, pl_ids = s.polyline_sets(max_sets=4)
    ctx.match_resident(b, e, device_only=True)
    _, dv1, _ = ctx.replay_device(to_host=False)
    with_one_shot = ctx.match_polyline_sets(n_sets, row_off, pl_ids, matched=dv1)
    plain = ctx.match_polyline_sets(n_sets, row_off, pl_ids)
    r = _ranges(b, e, 3)
    ctx.match_resident(*r[0], device_only=True)
    ctx.replay_accumulate(None, reset=True, materialise=False)            # cloud 0
    dv, n, pr = _shard_graph(clones[0], *r[1])
    ctx.replay_merge(dv, n, pr, materialise=False)                        # the graph of cloud 1
    ctx.match_resident(*r[2], device_only=True)
    got, dva, st = ctx.replay_accumulate(None)                            # cloud 2
    _check_step(ctx, got, dva, st, want, st1["n_pairs"], cloud["n_points"], "mixture")
    got_cloud = ctx.match_polyline_sets(n_sets, row_off, pl_ids, matched=dva)
    assert got_cloud["n_points"] == with_one_shot["n_points"] > 0
    for f in ("X", "obs_off", "obs_view", "obs_pl", "obs_seg", "obs_xy", "key"):
        assert got_cloud[f].tobytes() == with_one_shot[f].tobytes(), f
    assert plain["n_points"] != with_one_shot["n_points"], "the matched intervals change nothing on these sets"


# ---- 4. a host graph, uploaded -----------------------------------------------------------------------------------------------------
def test_a_host_graph_dict_merges_like_a_device_graph(eg3d_form, small):
    sa, o, clouds = small
    scene = C.byref(sa.c)
    ctx = api.Context(scene)
    try:
        for name in ("b_both_orientations", "e_first_interval_wins", "g_shared_extreme", "i_one_point_chains"):
            cloud = clouds[name]
            parts = parts_at(cloud, chain_starts(cloud))
            for i, p in enumerate(parts):
                got, dv, st = ctx.replay_merge(host.replay_matches(scene, p), p["n_points"], _n_pairs(p), reset=(i == 0))
                cat = concat(parts[:i + 1])
                _check_step(ctx, got, dv, st, o.replay_matches(cat), _n_pairs(cat), cat["n_points"], (name, i))
    finally:
        ctx.close()


# ---- 5. refusals leave the state, the outputs and the stats as they were ------------------------------------------------------------
def test_every_refusal_leaves_the_state_as_it_was(eg3d_form):
    sa = mc.scene_with_an_invalid_polyline()
    scene = C.byref(sa.c)
    o = ob.Oracle(scene)
    clouds = rc.cases()
    first, f = clouds["a_shared_node"], clouds["f_same_segment"]
    good = host.replay_matches(scene, f)
    L = api.lib()
    ctx = api.Context(scene)
    try:
        empty = rc.upload_cloud(ctx, slice_cloud(first, 0, 0))

        def raw(later, n_points, reset):
            """The call with every output given: (code, outputs untouched)."""
            dv, g, st = D.DeviceGraph3D(), D.Graph3D(), D.ReplayStats()
            st.struct_size, st.n_pairs, st.n_nodes, dv.n_nodes, g.n_nodes = C.sizeof(D.ReplayStats), 77, 78, 79, 80
            code = L.eg3d_replay_merge_graph(ctx._h, C.byref(later) if later is not None else None, n_points, 5, reset,
                                             C.byref(dv), C.byref(g), C.byref(st))
            return code, (st.n_pairs, st.n_nodes, dv.n_nodes, g.n_nodes, bool(g.node_X), bool(dv.node_X)) == (77, 78, 79, 80, False, False)

        def state():
            got, dv, st = ctx.replay_accumulate(empty[0])
            return got, dv, st

        ctx.replay_merge(host.replay_matches(scene, first), first["n_points"], _n_pairs(first), reset=True)
        accepted = [first]
        cases = mc.refused_graphs(good, f["n_points"]) + [
            ("the points of the run would reach 0xfffffff0", good, 0xfffffff0 - first["n_points"], mc.ERR_CAPACITY)]
        for i, (what, bad, n_points, code) in enumerate(cases):
            later, held = ctx.upload_graph(bad)
            # every other one asks for a reset, which must not happen (but the capacity case: it counts the points so far)
            got_code, untouched = raw(later, n_points, i % 2 if code != mc.ERR_CAPACITY else 0)
            assert got_code == code, (what, got_code)
            assert untouched and L.eg3d_last_error(), what
            cat = concat(accepted)
            got, dv, st = state()
            _check_step(ctx, got, dv, st, o.replay_matches(cat), _n_pairs(cat), cat["n_points"], what)
            # the next valid merge continues from what was accepted
            got, dv, st = ctx.replay_merge(good, f["n_points"], _n_pairs(f))
            accepted.append(f)
            cat = concat(accepted)
            _check_step(ctx, got, dv, st, o.replay_matches(cat), _n_pairs(cat), cat["n_points"], what)
        # null arguments, and the accumulator's own graph
        assert raw(None, 8, 0) == (mc.ERR_ARG, True)
        later, held = ctx.upload_graph(good)
        assert L.eg3d_replay_merge_graph(None, C.byref(later), 8, 0, 0, None, None, None) == mc.ERR_ARG
        got, own, st = state()
        assert raw(own, cat["n_points"], 0) == (mc.ERR_ARG, True)
        got, dv, st = state()
        _check_step(ctx, got, dv, st, o.replay_matches(cat), _n_pairs(cat), cat["n_points"], "after the last refusals")
        # the capacity case needs no memory: it is judged from later_points before anything is read
        wild = D.DeviceGraph3D()
        wild.n_nodes = wild.n_polylines = 1 << 40
        wild.n_scene_polylines = int(later.n_scene_polylines)
        assert raw(wild, 0xfffffff0, 0) == (mc.ERR_CAPACITY, True)
    finally:
        ctx.close()


# ---- 6. table growth, in a child process (EG3D_REPLAY_TABLE_BITS is read when a context is created) ---------------------------------
def test_the_merge_rehashes_from_sixteen_slots_in_a_child_process(eg3d_form, shards, tmp_path):
    s, ctx, clones, (b, e), cloud, want, one_shot, st1 = shards.items["c2_window"]
    out = tmp_path / "merged.npz"
    env = dict(os.environ, EG3D_REPLAY_TABLE_BITS="4")
    subprocess.run([sys.executable, os.path.join(HERE, "replay_merge_child.py"), str(out)], env=env, check=True, timeout=300)
    z = np.load(out)
    got = {f: (int(z[f]) if f in rc.FIELDS else z[f]) for f in rc.FIELDS + rc.ARRAYS}
    assert rc.same_graph(got, want) is None, rc.same_graph(got, want)
    slots, nodes = [int(x) for x in z["slots"]], [int(x) for x in z["shard_nodes"]]
    assert int(z["pairs"]) == st1["n_pairs"] and slots[0] >= 16
    for i, sl in enumerate(slots):      # after every merge: the power of two above twice the nodes of the graphs merged so far
        assert sl == max(16, 1 << (2 * sum(nodes[:i + 1])).bit_length()), (slots, nodes)
    assert slots[-1] > slots[0] and slots[-1] > 2 * want["n_nodes"]


# ---- 7. nothing stays behind ----------------------------------------------------------------------------------------------------------
def test_live_device_bytes_return_after_the_contexts_close(eg3d_form, small):
    sa, o, clouds = small
    before = _live()
    pool = Pool(C.byref(sa.c), 3)
    try:
        acc, w = pool.take(), pool.take()
        cloud = clouds["g_shared_extreme"]
        for i, p in enumerate(parts_at(cloud, chain_starts(cloud))):
            dvp, n, pr, held = _replayed(w, p)
            got, dv, st = acc.replay_merge(dvp, n, pr, reset=(i == 0))
        assert rc.same_graph(got, o.replay_matches(cloud)) is None
        got, dv, st = acc.replay_merge(got, cloud["n_points"], reset=True)         # an uploaded graph frees its arrays too
        assert _live() > before
        del held, dvp, dv
    finally:
        pool.close()
    import gc
    gc.collect()
    assert _live() == before
