"""The matches manager merges the GRAPHS of later shards, host form (include/eg3d_host_replay_merge.h), without a GPU: a
state that takes, in place of the clouds of a run, the graphs that separate replays of them built must hold after every
merge the graph the oracle's replay_matches builds from the concatenation of those clouds — as a left fold and as a pairwise
tree. The reference is never the merge itself. Every comparison is exact (replay_gpu_cases.same_graph). Also here: every
refusal. (The two headers against their tables: tests/test_abi.py.)"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import forms
import replay_gpu_cases as rc
import replay_merge_cases as mc
from edgegraph3d_amd import _cdefs as D, build, host
from oracle import binding as ob
from test_replay_accumulate import chain_starts, concat, parts_at, slice_cloud, _ranges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def small():
    sa = rc.small_scene()
    return sa, ob.Oracle(C.byref(sa.c)), rc.cases()


# ---- 1. hand-built clouds, every subset of their chain boundaries, fold and tree -------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_every_cut_of_a_hand_built_cloud(small, name):
    sa, o, clouds = small
    cloud, scene = clouds[name], C.byref(sa.c)
    whole = o.replay_matches(cloud)
    starts = chain_starts(cloud)
    graph_of = lambda p: host.replay_matches(scene, p)
    n_folds = 0
    for r in range(len(starts) + 1):
        for cuts in itertools.combinations(starts, r):
            parts = parts_at(cloud, cuts)
            if len(parts) > 1:
                parts = parts[:1] + [slice_cloud(cloud, 0, 0)] + parts[1:]      # an empty part in the middle changes nothing
            wants = {}

            def check(st, lo, hi):
                if (lo, hi) not in wants:
                    wants[(lo, hi)] = o.replay_matches(concat(parts[lo:hi]))
                g = st.graph()
                assert rc.same_graph(g, wants[(lo, hi)]) is None, (name, cuts, lo, hi, rc.same_graph(g, wants[(lo, hi)]))
                assert st.n_points == sum(p["n_points"] for p in parts[lo:hi])

            st = mc.fold(lambda: host.ReplayState(scene), parts, graph_of, check)
            try:
                assert rc.same_graph(st.graph(), whole) is None, (name, cuts)
            finally:
                st.close()
            g, n = mc.tree(lambda: host.ReplayState(scene), lambda s: s.close(), parts, graph_of, check)
            assert n == cloud["n_points"] and rc.same_graph(g, whole) is None, (name, cuts, "tree", rc.same_graph(g, whole))
            n_folds += 1
    assert n_folds == 2 ** len(starts)
    if name == "a_shared_node":      # the node whose last point lies in the later part, the shard's number rebased
        assert whole["node_point"].tolist() == [3, 1, 2]


def test_merging_into_an_empty_state_yields_the_graph_itself(small):
    sa, o, clouds = small
    scene = C.byref(sa.c)
    for name, cloud in clouds.items():
        g = host.replay_matches(scene, cloud)
        st = host.ReplayState(scene)
        try:
            st.merge(g, cloud["n_points"])
            assert rc.same_graph(st.graph(), g) is None, name
            conn_free = {k: v for k, v in g.items() if not k.startswith("conn_")}       # conn_* are not read
            conn_free["conn_off"], conn_free["conn_pl"] = np.zeros(0, np.uint64), np.zeros(0, np.uint32)
            st2 = host.ReplayState(scene)
            st2.merge(conn_free, cloud["n_points"])
            assert rc.same_graph(st2.graph(), g) is None, name
            st2.close()
        finally:
            st.close()


# ---- 2. the oracle's clouds by seed range ------------------------------------------------------------------------------------------
_MATCHED = {}


def _range_clouds(rows, cfg, b, e):
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
        whole = o.replay_matches(clouds[(b, e)])
        for k in (2, 3, 5):
            parts = [clouds[r] for r in _ranges(b, e, k)]
            assert sum(p["n_points"] for p in parts) == clouds[(b, e)]["n_points"]
            graphs = [o.replay_matches(p) for p in parts]           # the shards' graphs are the oracle's too
            separate = sum(_totals(g) for g in graphs)
            print("form %d config %d, %d shards: whole %s, sum of the separate graphs %s" % (rows, cfg, k, _totals(whole), separate))
            if cfg == 2:
                # the condition: concatenating the shards' graphs would NOT pass
                assert (separate > _totals(whole)).all(), (separate, _totals(whole))
            if cfg == 2 and k == 2 and rows == 3:
                assert separate.tolist() == [29249, 28436, 30905] and _totals(whole).tolist() == [29229, 28420, 22174]
            by_id = {id(p): g for p, g in zip(parts, graphs)}
            graph_of = lambda p: by_id[id(p)]
            last = {}

            def check(st, lo, hi):
                last["g"] = st.graph()

            st = mc.fold(lambda: host.ReplayState(s.scene), parts, graph_of, check)
            try:
                assert rc.same_graph(last["g"], whole) is None, (k, "fold", rc.same_graph(last["g"], whole))
                assert st.n_points == clouds[(b, e)]["n_points"]
            finally:
                st.close()
            g, n = mc.tree(lambda: host.ReplayState(s.scene), lambda x: x.close(), parts, graph_of, check)
            assert rc.same_graph(g, whole) is None, (k, "tree", rc.same_graph(g, whole))


# ---- 3. clouds and graphs mixed ------------------------------------------------------------------------------------------------------
def test_a_mixture_of_clouds_and_graphs(small):
    sa, o, clouds = small
    scene = C.byref(sa.c)
    parts = [clouds["a_shared_node"], clouds["e_first_interval_wins"], clouds["b_both_orientations"], clouds["g_shared_extreme"]]
    st = host.ReplayState(scene)
    try:
        st.add(parts[0])
        st.merge(host.replay_matches(scene, parts[1]), parts[1]["n_points"])
        assert rc.same_graph(st.graph(), o.replay_matches(concat(parts[:2]))) is None
        st.add(parts[2])
        assert rc.same_graph(st.graph(), o.replay_matches(concat(parts[:3]))) is None
        st.merge(host.replay_matches(scene, parts[3]), parts[3]["n_points"])
        assert rc.same_graph(st.graph(), o.replay_matches(concat(parts))) is None
        assert st.n_points == sum(p["n_points"] for p in parts)
        # the cut-chain check is skipped for the first cloud after a merge (a graph does not carry the last key) ...
        cont = slice_cloud(clouds["c_loop"], 2, 5)
        st.add(cont)
        # ... and stands again after it
        with pytest.raises(ValueError):
            st.add({**cont, "key": cont["key"] + np.array([0, 0, 0, 3], np.uint32)})
    finally:
        st.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_state_as_it_was():
    sa = mc.scene_with_an_invalid_polyline()
    scene = C.byref(sa.c)
    o = ob.Oracle(scene)
    clouds = rc.cases()
    first, f = clouds["a_shared_node"], clouds["f_same_segment"]
    good = host.replay_matches(scene, f)
    st = host.ReplayState(scene)
    try:
        st.merge(host.replay_matches(scene, first), first["n_points"])
        accepted = [first]
        before = st.graph()
        cases = mc.refused_graphs(good, f["n_points"]) + [
            ("the points of the run would reach 0xfffffff0", good, 0xfffffff0 - first["n_points"], mc.ERR_CAPACITY)]
        for what, bad, n_points, code in cases:
            with pytest.raises(ValueError) as ex:
                st.merge(bad, n_points)
            assert ex.value.code == code, (what, ex.value.code)
            assert st.n_points == sum(p["n_points"] for p in accepted), what
            assert rc.same_graph(st.graph(), before) is None, what
            # the next valid merge continues from what was accepted
            st.merge(good, f["n_points"])
            accepted.append(f)
            before = st.graph()
            assert rc.same_graph(before, o.replay_matches(concat(accepted))) is None, what
        L = host.lib()
        ga = D.Graph3DArrays(good)
        assert L.eg3d_host_replay_state_merge_graph(None, C.byref(ga.c), 8) == mc.ERR_ARG
        assert L.eg3d_host_replay_state_merge_graph(st._h, None, 8) == mc.ERR_ARG
        assert rc.same_graph(st.graph(), before) is None
    finally:
        st.close()
    # a graph whose arrays are not as long as its counts say never reaches the library
    short = mc.copy_graph(good)
    short["iv_start_seg"] = short["iv_start_seg"][:-1]
    with pytest.raises(ValueError):
        D.Graph3DArrays(short)


def test_a_state_with_wiped_or_nan_nodes_refuses_a_graph(small):
    sa, o, clouds = small
    scene = C.byref(sa.c)
    ob0 = [(0, rc.P0, 0, 12, 10)]
    good = host.replay_matches(scene, clouds["a_shared_node"])
    for odd in ((np.nan, 2.0, 3.0), (-1.0, 2.0, 3.0)):
        cloud = rc.make_cloud([(rc.A, ob0, (0, 0, 0, 0)), (odd, ob0, (0, 0, 0, 1))])
        st = host.ReplayState(scene)
        try:
            st.add(cloud)
            before = st.graph()
            with pytest.raises(ValueError) as ex:
                st.merge(good, 4)
            assert ex.value.code == mc.ERR_HOSTONLY
            assert rc.same_graph(st.graph(), before) is None and st.n_points == 2
        finally:
            st.close()


def test_the_stand_alone_fold_through_the_c_entry_points(tmp_path):
    """tests/refapi/replay_merge_check.cpp: clouds added, graphs merged and halves merged hold the same bytes after every
    step, refusals in between (the program that is also run under -fsanitize=address,undefined; no GPU, no Python)."""
    exe = str(tmp_path / "replay_merge_check")
    pkg = os.path.dirname(build.HOST_LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "refapi", "replay_merge_check.cpp"), "-L", pkg, "-leg3d_host",
                           "-Wl,-rpath," + pkg, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "replay_merge_check 0" in r.stdout, (r.stdout, r.stderr)
