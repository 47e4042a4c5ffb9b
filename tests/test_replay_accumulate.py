"""The matches manager that accumulates over calls, host form (include/eg3d_host_accumulate.h), without a GPU: a state fed
the parts of a cloud must hold, after every add, the graph host.replay_matches and the oracle's replay_matches build from the
concatenation of the parts so far. Every comparison is exact (replay_gpu_cases.same_graph). Also here: the reference-API
shim's set_accumulate. (The two headers against their tables: tests/test_abi.py.)"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import cbuild
import forms
import replay_gpu_cases as rc
from edgegraph3d_amd import host
from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUD_ARRAYS = ("X", "obs_view", "obs_pl", "obs_seg", "obs_xy", "key")


def slice_cloud(cloud, a, b):
    """Points [a, b) of a cloud dict as a cloud of its own (obs_off with its sentinel, counted from 0)."""
    off = cloud["obs_off"]
    o0, o1 = (int(off[a]), int(off[b])) if cloud["n_points"] else (0, 0)
    out = {"n_points": b - a, "n_obs": o1 - o0, "obs_off": (off[a:b + 1] - off[a]).astype(off.dtype) if cloud["n_points"]
           else off.copy()}
    for f in ("X", "key"):
        out[f] = cloud[f][a:b].copy()
    for f in ("obs_view", "obs_pl", "obs_seg", "obs_xy"):
        out[f] = cloud[f][o0:o1].copy()
    return out


def chain_starts(cloud):
    """The indices 1 .. n - 1 at which a new chain begins: where a cloud may be cut."""
    k = cloud["key"].astype(np.int64).reshape(-1, 4)
    return [i for i in range(1, len(k))
            if not (np.array_equal(k[i, :3], k[i - 1, :3]) and k[i, 3] == (k[i - 1, 3] + 1) % 2**32)]


def parts_at(cloud, cuts):
    edges = [0] + list(cuts) + [cloud["n_points"]]
    return [slice_cloud(cloud, a, b) for a, b in zip(edges[:-1], edges[1:])]


def concat(parts):
    """The concatenation the contract speaks of (observation offsets counted through)."""
    out = {"n_points": sum(p["n_points"] for p in parts), "n_obs": sum(p["n_obs"] for p in parts)}
    for f in CLOUD_ARRAYS:
        out[f] = np.concatenate([p[f] for p in parts])
    off, base = [np.zeros(1, parts[0]["obs_off"].dtype)], 0
    for p in parts:
        off.append(p["obs_off"][1:] + np.asarray(base, p["obs_off"].dtype))
        base += p["n_obs"]
    out["obs_off"] = np.concatenate(off)
    return out


@pytest.fixture(scope="module")
def small():
    """The three-view scene of the hand-built cases, its oracle, the clouds and the oracle's graph of each whole cloud."""
    sa = rc.small_scene()
    o = ob.Oracle(C.byref(sa.c))
    clouds = rc.cases()
    return sa, o, clouds, {k: o.replay_matches(v) for k, v in clouds.items()}


# ---- 1. hand-built clouds, every subset of their chain boundaries ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_every_cut_of_a_hand_built_cloud(small, name):
    sa, o, clouds, wants = small
    cloud, scene = clouds[name], C.byref(sa.c)
    whole = host.replay_matches(scene, cloud)
    assert rc.same_graph(whole, wants[name]) is None
    starts = chain_starts(cloud)
    n_cuts = 0
    for r in range(len(starts) + 1):
        for cuts in itertools.combinations(starts, r):
            parts = parts_at(cloud, cuts)
            # ... and once more with an empty cloud put in the middle, which must change nothing
            for with_empty in ((False, True) if len(parts) > 1 else (False,)):
                fed = parts[:1] + [slice_cloud(cloud, 0, 0)] + parts[1:] if with_empty else parts
                st = host.ReplayState(scene)
                try:
                    so_far = []
                    for p in fed:
                        st.add(p)
                        so_far.append(p)
                        g = st.graph()
                        want = o.replay_matches(concat(so_far))
                        assert rc.same_graph(g, want) is None, (name, cuts, len(so_far), rc.same_graph(g, want))
                        assert rc.same_graph(g, host.replay_matches(scene, concat(so_far))) is None, (name, cuts)
                        assert rc.same_graph(st.graph(), g) is None       # asking does not disturb the state
                    assert st.n_points == cloud["n_points"]
                    assert rc.same_graph(st.graph(), whole) is None, (name, cuts, rc.same_graph(st.graph(), whole))
                finally:
                    st.close()
            n_cuts += 1
    assert n_cuts == 2 ** len(starts)
    if name in ("a_shared_node", "b_both_orientations", "d_signed_zero", "e_first_interval_wins", "g_shared_extreme", "j_key_gap"):
        assert starts, name      # these carry what matters across a cut: they must have one
    if name == "a_shared_node":   # the node whose last point lies in the later part
        assert whole["node_point"].tolist() == [3, 1, 2]


# ---- 2. the oracle's clouds by seed range ------------------------------------------------------------------------------------
def _ranges(b, e, k):
    edges = [b + (e - b) * i // k for i in range(k + 1)]
    return list(zip(edges[:-1], edges[1:]))


_MATCHED = {}


def _range_clouds(rows, cfg, b, e):
    """(synth, oracle, {(b, e): cloud}) with the oracle's cloud of every range the 1-, 2-, 3- and 5-step cuts need; computed
    once per form and never modified."""
    if (rows, cfg) not in _MATCHED:
        with forms.oracle_rows(rows):
            s = host.Synth(cfg)
            o = ob.Oracle(s.scene)
            e = s.n_seeds if e is None else e
            clouds = {}
            for k in (1, 2, 3, 5):
                for r in _ranges(b, e, k):
                    if r not in clouds:
                        clouds[r] = o.match(s.seeds, r[0], r[1], os.cpu_count() and min(16, os.cpu_count()) or 1)
            _MATCHED[(rows, cfg)] = (s, o, clouds, (b, e))
    return _MATCHED[(rows, cfg)]


def _totals(g):
    return np.array([g["n_nodes"], g["n_polylines"], int(g["iv_off"][-1])])


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
@pytest.mark.parametrize("cfg,b,e", [(0, 0, None), (2, 1550, 1800)], ids=["config0", "c2_window"])
def test_oracle_clouds_by_seed_range(rows, cfg, b, e):
    s, o, clouds, (b, e) = _range_clouds(rows, cfg, b, e)
    with forms.oracle_rows(rows):
        whole_cloud = clouds[(b, e)]
        whole = o.replay_matches(whole_cloud)
        assert rc.same_graph(host.replay_matches(s.scene, whole_cloud), whole) is None
        for k in (2, 3, 5):
            parts = [clouds[r] for r in _ranges(b, e, k)]
            cat = concat(parts)
            for f in CLOUD_ARRAYS + ("obs_off",):      # the steps' clouds ARE the one-call cloud, cut
                assert np.array_equal(cat[f].view(np.uint32) if cat[f].dtype.kind == "f" else cat[f],
                                      whole_cloud[f].view(np.uint32) if cat[f].dtype.kind == "f" else whole_cloud[f]), f
            separate = sum(_totals(o.replay_matches(p)) for p in parts)
            print("form %d config %d, %d steps: whole %s, sum of the separate replays %s" % (rows, cfg, k, _totals(whole), separate))
            if cfg == 2:
                # the condition: replaying each step and concatenating the graphs would NOT pass
                assert (separate > _totals(whole)).all(), (separate, _totals(whole))
                assert (separate - _totals(whole))[:2].tolist() == [20, 16]
            st = host.ReplayState(s.scene)
            try:
                for i, p in enumerate(parts):
                    st.add(p)
                    if k == 3:    # the intermediate graphs too (one k: the oracle's replay of a prefix is not free)
                        want = o.replay_matches(concat(parts[:i + 1]))
                        assert rc.same_graph(st.graph(), want) is None, (k, i, rc.same_graph(st.graph(), want))
                g = st.graph()
                assert rc.same_graph(g, whole) is None, (k, rc.same_graph(g, whole))
                assert st.n_points == whole_cloud["n_points"]
            finally:
                st.close()
        if cfg == 2:
            want = {3: (29229, 28420, 22174), 2: (29223, 28414, 21883)}[rows]
            assert tuple(_totals(whole)) == want


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------
def test_a_cut_inside_a_chain_is_refused_and_the_state_stands(small):
    sa, o, clouds, wants = small
    cloud, scene = clouds["c_loop"], C.byref(sa.c)
    assert 2 not in chain_starts(cloud)
    first, second = slice_cloud(cloud, 0, 2), slice_cloud(cloud, 2, cloud["n_points"])
    st = host.ReplayState(scene)
    try:
        st.add(first)
        before = st.graph()
        with pytest.raises(ValueError):
            st.add(second)
        assert st.n_points == 2
        assert rc.same_graph(st.graph(), before) is None and rc.same_graph(before, o.replay_matches(first)) is None
        # a cloud the scene does not fit is refused the same way ...
        bad = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in clouds["a_shared_node"].items()}
        bad["obs_seg"][0] = 99
        with pytest.raises(ValueError):
            st.add(bad)
        assert rc.same_graph(st.graph(), before) is None
        # ... and the next valid cloud continues from what was accepted
        nxt = clouds["j_key_gap"].copy()
        nxt["key"] = nxt["key"] + np.array([5, 0, 0, 0], np.uint32)
        st.add(nxt)
        want = o.replay_matches(concat([first, nxt]))
        assert rc.same_graph(st.graph(), want) is None
    finally:
        st.close()


def test_nan_and_invalid_coordinates_across_clouds(small):
    """The host form keeps the reference's treatment of NaN and -1 (a node per lookup; the invalid-node wipe), also when
    the lookups that meet lie in different clouds."""
    sa, o, clouds, wants = small
    scene = C.byref(sa.c)
    nan, inv = (np.nan, 2.0, 3.0), (-1.0, 2.0, 3.0)
    ob0 = [(0, rc.P0, 0, 12, 10)]
    cloud = rc.make_cloud([
        (rc.A, ob0, (0, 0, 0, 0)), (nan, ob0, (0, 0, 0, 1)), (rc.B, ob0, (0, 0, 0, 2)),
        (inv, ob0, (1, 0, 0, 0)), (rc.A, ob0, (1, 0, 0, 1)),
        (inv, ob0, (2, 0, 0, 0)), (nan, ob0, (2, 0, 0, 1)), (rc.B, [], (2, 0, 0, 2)),
        (rc.A, ob0, (3, 0, 0, 0)), (inv, ob0, (3, 0, 0, 1))])
    whole = o.replay_matches(cloud)
    assert rc.same_graph(host.replay_matches(scene, cloud), whole) is None
    assert whole["n_nodes"] > whole["n_real_nodes"] or whole["n_nodes"] > 4     # the wipe or the NaN nodes took place
    starts = chain_starts(cloud)
    assert starts == [3, 5, 8]
    for r in range(len(starts) + 1):
        for cuts in itertools.combinations(starts, r):
            st = host.ReplayState(scene)
            try:
                for p in parts_at(cloud, cuts):
                    st.add(p)
                g = st.graph()
                assert g["n_real_nodes"] == whole["n_real_nodes"]
                assert rc.same_graph(g, whole) is None, (cuts, rc.same_graph(g, whole))
            finally:
                st.close()


# ---- 4. the reference-API shim -------------------------------------------------------------------------------------------------
def test_shim_manager_accumulates_when_asked(tmp_path):
    """tests/refapi/accumulate_check.cpp: two replay_chains calls with set_accumulate(true) == one call with all the chains;
    with the default setting the second call replaces; and the host state driven by hand (no GPU is touched)."""
    exe = cbuild.build_caller("tests/refapi/accumulate_check.cpp", tmp_path, lib=cbuild.DEFAULT_LIB)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "accumulate_check 0" in r.stdout, (r.stdout, r.stderr)
