"""-m gpu: the PLGMatchesManager replay on a device-resident cloud (eg3d_replay_device). Every graph is compared field for
field and bit for bit with the oracle's replay (orc_replay_matches, the reference's containers) of the host copy of the very
same cloud; the graph copied back from the device view by the test must equal the library's host copy."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import replay_gpu_cases as rc
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host
from edgegraph3d_amd.cloudnp import np_compact
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_HOSTONLY = -1, -3, -5
_CACHE = {}


class Matched:
    """Per DLT form: contexts on synthetic config 0 (whole) and on a seed window of C2, their clouds left in HBM by a
    device-only match, the host copies and the oracle's graphs (computed once, never modified). The window: C2's seeds are
    mostly far apart, and its chains share nodes only where two seeds lie on one curve point; seeds 1550-1799 hold such
    seeds (27 shared nodes and 20 repeated connections in the oracle's cloud of that range; the first eighth of the seeds
    has none)."""

    def __init__(self):
        assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
        self.items = {}
        for name, cfg, window in (("config0", 0, None), ("c2_window", 2, (1550, 1800))):
            s = host.Synth(cfg)
            ctx = api.Context(s.scene)
            ctx.upload_seeds(s.seeds)
            begin, end = (0, s.n_seeds) if window is None else window
            r = ctx.match_resident(begin, end, device_only=True)
            dev = ctx.last_device_output()
            assert dev.complete == 1 and int(dev.n_points) == r["n_points"] > 100
            cloud = ctx.fetch_device_output()
            self.items[name] = (s, ctx, dev, cloud, ob.Oracle(s.scene).replay_matches(cloud))

    def close(self):
        for s, ctx, *_ in self.items.values():
            ctx.close()


def _drop_cache():
    import forms
    for rows, m in list(_CACHE.items()):
        with forms.product_form(rows):
            m.close()
    _CACHE.clear()


@pytest.fixture
def matched(eg3d_form):
    if eg3d_form not in _CACHE:
        _drop_cache()
        _CACHE[eg3d_form] = Matched()
    return _CACHE[eg3d_form]


@pytest.fixture(scope="module", autouse=True)
def _close_cached_contexts():
    yield
    _drop_cache()


@pytest.fixture(scope="module")
def small():
    """The three-view scene of the hand-built cases, its oracle and the oracle's graph of every case."""
    sa = rc.small_scene()
    o = ob.Oracle(C.byref(sa.c))
    clouds = rc.cases()
    return sa, clouds, {k: o.replay_matches(v) for k, v in clouds.items()}


def _pairs(cloud):
    k = cloud["key"].astype(np.int64)
    if len(k) < 2:
        return np.zeros(len(k), bool)
    p = np.all(k[1:, :3] == k[:-1, :3], axis=1) & (k[1:, 3] == (k[:-1, 3] + 1) % 2**32)
    return np.concatenate([[False], p])


def _check(ctx, dev, want, what):
    """One replay of `dev`: the host copy, the device view copied back by the test and the statistics against `want`."""
    got, dv, st = ctx.replay_device(dev)
    print("%s: %d pairs -> %d nodes, %d polylines, %d intervals; table %d slots; graph %.3f ms, intervals %.3f ms, copy %.3f ms"
          % (what, st["n_pairs"], st["n_nodes"], st["n_polylines"], st["n_intervals"], st["table_slots"], st["ms_graph"],
             st["ms_intervals"], st["ms_copy"]))
    assert rc.same_graph(got, want) is None, (what, rc.same_graph(got, want))
    back = ctx.fetch_device_graph(dv)
    assert rc.same_graph(back, got) is None, (what, "device view", rc.same_graph(back, got))
    assert int(dv.n_scene_polylines) == len(want["iv_off"]) - 1 == len(got["iv_off"]) - 1
    assert st["struct_size"] == C.sizeof(D.ReplayStats)
    assert (st["n_nodes"], st["n_polylines"], st["n_intervals"]) == (want["n_nodes"], want["n_polylines"], int(want["iv_off"][-1]))
    return got, st


# ---- 1. matched clouds ----
@pytest.mark.parametrize("name", ["config0", "c2_window"])
def test_matched_cloud_against_the_oracle(matched, name):
    s, ctx, dev, cloud, want = matched.items[name]
    got, st = _check(ctx, None, want, name)                      # NULL = the context's last device output
    pairs = _pairs(cloud)
    in_pairs = int((pairs | np.concatenate([pairs[1:], [False]])).sum())
    assert st["n_pairs"] == int(pairs.sum()) > 0 and got["n_polylines"] > 0 and got["iv_off"][-1] > 0
    assert got["n_nodes"] <= in_pairs
    if name == "c2_window":
        assert got["n_nodes"] < in_pairs, "the chains of the window share no node: the test would pass vacuously"
        assert got["n_polylines"] < st["n_pairs"], "no connection of the window repeats"
    _check(ctx, dev, want, name + " (explicit view)")


@pytest.mark.parametrize("name", ["config0", "c2_window"])
def test_compacted_cloud_against_the_oracle(matched, name):
    s, ctx, dev, cloud, _ = matched.items[name]
    keep, n_kept = ctx.dedup_device(dev)
    comp = ctx.compact_device(dev, keep)
    assert 0 < int(comp.n_points) == n_kept < cloud["n_points"]
    small_cloud = np_compact(cloud, keep.numpy(np.uint8)[:cloud["n_points"]])
    want = ob.Oracle(s.scene).replay_matches(small_cloud)        # (dropped points break chains: key[3] no longer counts up)
    _check(ctx, comp, want, name + " compacted")
    assert want["n_polylines"] > 0


# ---- 2. hand-built clouds ----
@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_hand_built_cloud(eg3d_form, small, name):
    sa, clouds, wants = small
    ctx = api.Context(C.byref(sa.c))
    try:
        d, held = rc.upload_cloud(ctx, clouds[name])
        g, st = _check(ctx, d, wants[name], name)
        gp = lambda view, pl: rc.global_pl(view, pl)
        iv = lambda p: list(zip(g["iv_start_seg"][int(g["iv_off"][p]):int(g["iv_off"][p + 1])].tolist(),
                                g["iv_end_seg"][int(g["iv_off"][p]):int(g["iv_off"][p + 1])].tolist()))
        pls = list(zip(g["pl_start"].tolist(), g["pl_end"].tolist()))
        conn = lambda n: g["conn_pl"][int(g["conn_off"][n]):int(g["conn_off"][n + 1])].tolist()
        # what the case is about, stated beside the comparison with the oracle so that a failure names the rule
        if name == "a_shared_node":
            assert g["n_nodes"] == 3 and g["node_point"].tolist() == [3, 1, 2] and pls == [(0, 1), (2, 0)]
            assert conn(0) == [0, 1]
        elif name == "b_both_orientations":
            assert pls == [(0, 1), (1, 2)] and conn(1) == [0, 1]
        elif name == "c_loop":
            assert pls == [(0, 0), (0, 1)] and conn(0) == [0, 1] and g["node_point"].tolist() == [4, 2]
        elif name == "d_signed_zero":
            assert g["n_nodes"] == 2 and g["node_X"].view(np.uint32)[0, 0] == 0x80000000 and pls == [(0, 1), (0, 0)]
        elif name == "e_first_interval_wins":
            assert iv(gp(0, rc.P0)) == [(0, 2)] and iv(gp(1, rc.Q0)) == [(0, 2)]
        elif name == "f_same_segment":
            a = int(g["iv_off"][gp(0, rc.P0)])
            assert iv(gp(0, rc.P0)) == [(1, 1), (2, 2)] and g["iv_start_xy"][a:a + 2].tolist() == [[22, 10], [32, 10]]
            assert g["iv_start_xy"][int(g["iv_off"][gp(0, rc.P1)])].tolist() == [62, 22]
        elif name == "g_shared_extreme":
            assert iv(gp(0, rc.P2)) == [(0, 1)] and iv(gp(0, rc.P1)) == [(0, 1)] and st["n_intervals"] == 2
            assert g["iv_end_xy"][int(g["iv_off"][gp(0, rc.P2)])].tolist() == [10, 10]      # P2's last vertex, as the END
            assert g["iv_start_xy"][int(g["iv_off"][gp(0, rc.P1)])].tolist() == [50, 10]    # P1's first vertex
        elif name == "h_repeated_view":
            assert iv(gp(0, rc.P0)) == [(0, 2)] and iv(gp(1, rc.Q0)) == [(0, 1)]
        elif name.startswith("i_"):
            assert (g["n_nodes"], g["n_polylines"], st["n_pairs"], st["n_intervals"]) == (0, 0, 0, 0)
            assert len(g["iv_off"]) == sum(len(v) for v in rc.POLYLINES) + 1 and not g["iv_off"].any()
            assert g["conn_off"].tolist() == [0]
        elif name == "j_key_gap":
            assert st["n_pairs"] == 1 and g["n_nodes"] == 2 and g["node_X"].tolist() == [list(rc.B), list(rc.Cc)]
    finally:
        ctx.close()


# ---- 3. table stress ----
def test_smallest_node_table_in_a_child_process(eg3d_form, matched, small, tmp_path):
    out = tmp_path / "graphs.npz"
    env = dict(os.environ, EG3D_REPLAY_TABLE_BITS="1")
    subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "replay_gpu_cases.py"), str(out)],
                   env=env, check=True, timeout=300)
    z = np.load(out)
    # the smallest table the library accepts: the power of two above the number of lookups (two per pair)
    for tag in ("0", "a"):
        lookups = 2 * int(z["pairs" + tag])
        assert int(z["slots" + tag]) == 1 << lookups.bit_length(), tag
    sa, clouds, wants = small
    for tag, want in (("c0", matched.items["config0"][4]), ("a", wants["a_shared_node"])):
        got = {f: (int(z[tag + "_" + f]) if f in rc.FIELDS else z[tag + "_" + f]) for f in rc.FIELDS + rc.ARRAYS}
        assert rc.same_graph(got, want) is None, (tag, rc.same_graph(got, want))
    # ... and the default table of this process is larger and gives the same graph
    s, ctx, dev, cloud, want = matched.items["config0"]
    _, st = _check(ctx, dev, want, "config0, default table")
    assert st["table_slots"] > int(z["slots0"])


# ---- 4. determinism ----
def test_two_replays_are_byte_identical(matched):
    s, ctx, dev, cloud, want = matched.items["c2_window"]
    g1, dv1, _ = ctx.replay_device(dev)
    b1 = ctx.fetch_device_graph(dv1)
    g2, dv2, _ = ctx.replay_device(dev)
    b2 = ctx.fetch_device_graph(dv2)
    for x, y in ((g1, g2), (b1, b2), (g1, b2)):
        assert rc.same_graph(x, y) is None
        for f in rc.ARRAYS:
            assert x[f].tobytes() == y[f].tobytes(), f


# ---- 5. refusals ----
def _raw(ctx, d, stats=None, dv=None, g=None):
    return api.lib().eg3d_replay_device(ctx._h, C.byref(d), C.byref(dv) if dv is not None else None,
                                        C.byref(g) if g is not None else None, C.byref(stats) if stats is not None else None)


def test_refusals_leave_the_context_usable(eg3d_form, small):
    sa, clouds, wants = small
    base = clouds["a_shared_node"]
    # a fifth point that belongs to no pair (a chain of its own): the host replay never looks it up
    lone = rc.make_cloud([(tuple(base["X"][i]), [(int(v), int(p), int(s), float(x), float(y)) for v, p, s, (x, y) in
                                                 zip(base["obs_view"][int(base["obs_off"][i]):int(base["obs_off"][i + 1])],
                                                     base["obs_pl"][int(base["obs_off"][i]):int(base["obs_off"][i + 1])],
                                                     base["obs_seg"][int(base["obs_off"][i]):int(base["obs_off"][i + 1])],
                                                     base["obs_xy"][int(base["obs_off"][i]):int(base["obs_off"][i + 1])])],
                           tuple(int(q) for q in base["key"][i])) for i in range(4)]
                         + [((9.0, 9.0, 9.0), [(2, rc.R0, 1, 40.0, 90.0)], (7, 0, 0, 0))])
    o = ob.Oracle(C.byref(sa.c))
    ctx = api.Context(C.byref(sa.c))

    def mutated(field, index, value):
        c = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in lone.items()}
        if field == "X":
            c["X"][index[0], index[1]] = value
        else:
            c[field][index] = value
        return c

    def valid_replay_succeeds():
        d, held = rc.upload_cloud(ctx, lone)
        _check(ctx, d, o.replay_matches(lone), "after a refusal")

    try:
        nv_p0 = len(rc.POLYLINES[0][rc.P0][0])
        refused = [
            ("NaN x of a paired point", mutated("X", (1, 0), np.nan), ERR_HOSTONLY),
            ("NaN z of a paired point", mutated("X", (3, 2), np.nan), ERR_HOSTONLY),
            ("x == -1 of a paired point", mutated("X", (0, 0), -1.0), ERR_HOSTONLY),
            ("y == -1 of a paired point", mutated("X", (2, 1), -1.0), ERR_HOSTONLY),
            ("view id == n_views", mutated("obs_view", 1, len(rc.POLYLINES)), ERR_ARG),
            ("view id < 0", mutated("obs_view", 4, -1), ERR_ARG),
            ("polyline id == the view's count", mutated("obs_pl", 0, len(rc.POLYLINES[0])), ERR_ARG),
            ("segment index == nv - 1", mutated("obs_seg", 0, nv_p0 - 1), ERR_ARG),
            ("descending offsets", mutated("obs_off", 2, 0), ERR_ARG),
            ("an offset beyond n_obs", mutated("obs_off", 4, lone["n_obs"] + 1), ERR_ARG),
        ]
        for what, cloud, code in refused:
            d, held = rc.upload_cloud(ctx, cloud)
            st, dv, g = D.ReplayStats(), D.DeviceGraph3D(), D.Graph3D()
            st.struct_size = C.sizeof(D.ReplayStats)
            st.n_pairs = dv.n_nodes = g.n_nodes = 12345
            assert _raw(ctx, d, st, dv, g) == code, what
            assert api.lib().eg3d_last_error(), what
            assert (st.n_pairs, dv.n_nodes, g.n_nodes) == (12345, 12345, 12345) and not g.node_X, what   # nothing written
            valid_replay_succeeds()
        # the same values in the point of no pair are never looked up: no refusal, and the oracle agrees on the graph
        for col, value in ((0, np.nan), (0, -1.0), (1, -1.0)):
            cloud = mutated("X", (4, col), value)
            d, held = rc.upload_cloud(ctx, cloud)
            _check(ctx, d, o.replay_matches(cloud), "lone point with %r" % value)
        # a struct_size that is too small is refused before anything is written
        d, held = rc.upload_cloud(ctx, lone)
        st, dv = D.ReplayStats(), D.DeviceGraph3D()
        st.struct_size = C.sizeof(D.ReplayStats) - 4
        st.n_pairs = dv.n_nodes = 777
        assert _raw(ctx, d, st, dv) == ERR_ARG and b"struct_size" in api.lib().eg3d_last_error()
        assert st.n_pairs == 777 and dv.n_nodes == 777 and st.struct_size == C.sizeof(D.ReplayStats) - 4
        valid_replay_succeeds()
        # ids are 32-bit: a point count the host replay refuses too (nothing is read: the check precedes every launch)
        big = D.DeviceEdgePoints()
        C.memmove(C.byref(big), C.byref(d), C.sizeof(big))
        big.n_points = 0xfffffff0
        assert _raw(ctx, big) == ERR_CAPACITY
        part = D.DeviceEdgePoints()
        C.memmove(C.byref(part), C.byref(d), C.sizeof(part))
        part.complete = 0
        assert _raw(ctx, part) == ERR_ARG
        valid_replay_succeeds()
    finally:
        ctx.close()


def test_graph_released_by_the_library_itself(eg3d_form, small):
    """eg3d_free_graph3d releases out_host and clears the struct; a second call on the cleared struct is harmless."""
    sa, clouds, wants = small
    ctx = api.Context(C.byref(sa.c))
    try:
        d, held = rc.upload_cloud(ctx, clouds["c_loop"])
        g = D.Graph3D()
        assert _raw(ctx, d, g=g) == 0 and g.n_nodes == 2 and g.node_X
        api.lib().eg3d_free_graph3d(C.byref(g))
        assert g.n_nodes == 0 and not g.node_X and not g.iv_off
        api.lib().eg3d_free_graph3d(C.byref(g))
    finally:
        ctx.close()

