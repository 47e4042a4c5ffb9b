"""What the tests of the matches manager's graph merge share (tests/test_replay_merge.py on the host statements,
tests/test_gpu_replay_merge.py on the device): the scene of the hand-built clouds with one invalid polyline behind it, the
graphs that every refusal of include/eg3d_replay_merge.h / include/eg3d_host_replay_merge.h names, and the fold and the
pairwise tree over the parts of a cut cloud."""
import numpy as np

import replay_gpu_cases as rc
from edgegraph3d_amd import host

ERR_ARG, ERR_CAPACITY, ERR_HOSTONLY = -1, -3, -5


def scene_with_an_invalid_polyline():
    """rc.small_scene() with a polyline without vertices (pl_valid = 0) behind view 2's: no global id of the hand-built
    clouds moves, and the last row of a graph's interval table belongs to a polyline that has no segments."""
    base = host.Synth(0).scene_np()
    V = len(rc.POLYLINES)
    vpo, pvo, vtx, ps, pe = [0], [0], [], [], []
    for view in rc.POLYLINES:
        for verts, a, b in view:
            vtx.extend(verts)
            pvo.append(len(vtx))
            ps.append(a)
            pe.append(b)
        vpo.append(len(ps))
    pvo.append(len(vtx)), ps.append(2), pe.append(3)
    vpo[-1] += 1
    valid = np.ones(len(ps), np.uint8)
    valid[-1] = 0
    return host.SceneArrays({
        "n_views": V, "width": base["width"], "height": base["height"], "cam_P": base["cam_P"][:V].copy(),
        "F": base["F"][:V, :V].copy(), "F_valid": base["F_valid"][:V, :V].copy(), "view_pl_off": np.array(vpo, np.uint32),
        "pl_vtx_off": np.array(pvo, np.uint32), "vtx_xy": np.array(vtx, np.float32), "pl_start": np.array(ps, np.uint32),
        "pl_end": np.array(pe, np.uint32), "pl_valid": valid})


def copy_graph(g):
    return {k: (v.copy() if hasattr(v, "copy") else v) for k, v in g.items()}


def with_scene_polylines(g, n):
    """The graph of a scene of n polylines from one of fewer: empty rows behind the last."""
    g = copy_graph(g)
    g["iv_off"] = np.concatenate([g["iv_off"], np.full(n + 1 - len(g["iv_off"]), g["iv_off"][-1], np.uint64)])
    return g


def refused_graphs(good, n_points):
    """[(what, graph, later_points, code)]: `good` — the graph of rc.cases()["f_same_segment"] over the scene above, 8 points:
    4 nodes, 4 polylines, two intervals on P0 (start segments 1 and 2), one on P1 and one on R0 — with one thing wrong each."""
    assert good["n_nodes"] == 4 and good["n_polylines"] == 4 and n_points == 8
    NP = len(good["iv_off"]) - 1
    assert good["iv_off"].tolist()[:3] == [0, 2, 3] and good["iv_start_seg"].tolist()[:2] == [1, 2]

    def mut(fn):
        g = copy_graph(good)
        fn(g)
        return g

    def set_(field, index, value):
        def fn(g):
            g[field][index] = value
        return fn

    def swap_first_two_intervals(g):
        for f in ("iv_start_seg", "iv_end_seg", "iv_start_xy", "iv_end_xy"):
            g[f][[0, 1]] = g[f][[1, 0]]

    def interval_on_the_invalid_polyline(g):      # the last row takes the interval that was R0's (the one before it)
        g["iv_off"][NP - 1] -= 1

    def same_pair_twice(g):
        g["pl_start"][1], g["pl_end"][1] = g["pl_end"][0], g["pl_start"][0]

    def signed_zeros(g):
        g["node_X"][0] = (0.0, 1.0, 1.0)
        g["node_X"][1] = (-0.0, 1.0, 1.0)

    def nan_and_bad_endpoint(g):
        g["node_X"][2, 2] = np.nan
        g["pl_end"][3] = 4

    def fewer_scene_polylines(g):
        g["iv_off"] = g["iv_off"][:-1].copy()

    A, H = ERR_ARG, ERR_HOSTONLY
    return [
        ("n_scene_polylines is not the scene's", mut(fewer_scene_polylines), 8, A),
        ("an endpoint that is no node", mut(set_("pl_end", 1, 4)), 8, A),
        ("a node_point that is no point of later", mut(set_("node_point", 0, 8)), 8, A),
        ("more nodes than points", copy_graph(good), 3, A),
        ("iv_off does not begin at 0", mut(set_("iv_off", 0, 1)), 8, A),
        ("iv_off descends", mut(set_("iv_off", 1, 4)), 8, A),
        ("a row longer than its polyline has segments", mut(set_("iv_off", 3, 9)), 8, A),
        ("a start segment outside its polyline", mut(set_("iv_start_seg", 1, 4)), 8, A),
        ("an end segment outside its polyline", mut(set_("iv_end_seg", 0, 4)), 8, A),
        ("an interval on an invalid polyline", mut(interval_on_the_invalid_polyline), 8, A),
        ("start segments that do not ascend", mut(swap_first_two_intervals), 8, A),
        ("start segments that repeat", mut(set_("iv_start_seg", 1, 1)), 8, A),
        ("two nodes with equal coordinates", mut(lambda g: g["node_X"].__setitem__(3, g["node_X"][0])), 8, A),
        ("two nodes that are -0 and +0", mut(signed_zeros), 8, A),
        ("two polylines on one pair of nodes", mut(same_pair_twice), 8, A),
        ("a NaN and a bad endpoint: the argument error comes first", mut(nan_and_bad_endpoint), 8, A),
        ("n_real_nodes != n_nodes", mut(lambda g: g.__setitem__("n_real_nodes", 3)), 8, H),
        ("a NaN coordinate", mut(set_("node_X", (2, 2), np.nan)), 8, H),
        ("x == -1", mut(set_("node_X", (0, 0), -1.0)), 8, H),
        ("y == -1", mut(set_("node_X", (1, 1), -1.0)), 8, H),
    ]


def fold(new_state, parts, graph_of, check):
    """Left fold: a fresh state takes graph_of(part) for every part in order; check(state, number of parts so far) after
    every merge. Returns the state."""
    st = new_state()
    for i, p in enumerate(parts):
        st.merge(graph_of(p), p["n_points"])
        check(st, 0, i + 1)
    return st


def tree(new_state, close, parts, graph_of, check, lo=0, hi=None):
    """Pairwise tree over parts[lo:hi]: (graph, points). A leaf is graph_of(part); an inner node is a fresh state that takes
    its left and then its right subtree; check(state, lo, hi) after every merge."""
    hi = len(parts) if hi is None else hi
    if hi - lo == 1:
        return graph_of(parts[lo]), parts[lo]["n_points"]
    mid = (lo + hi) // 2
    left, nl = tree(new_state, close, parts, graph_of, check, lo, mid)
    right, nr = tree(new_state, close, parts, graph_of, check, mid, hi)
    st = new_state()
    try:
        st.merge(left, nl)
        check(st, lo, mid)
        st.merge(right, nr)
        check(st, lo, hi)
        return st.graph(), nl + nr
    finally:
        close(st)
