"""CPU tests of pipeline 1's compatibility graph: the Python restatement (tests/simgraph_ref.py) on hand cases whose figures
are worked out here, the rank key of the node numbering, and the host side of the file seam (libeg3d_host.so) against the
restatement."""
import ctypes as C

import numpy as np
import pytest

import simgraph_cases as sc
import simgraph_ref as ref
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host

F32 = np.float32
ONE, W23, W37 = F32(1), F32(2) / F32(3), F32(3) / F32(7)   # an int divided by a float, as compute_refpoint_weight

_G = {}   # restatement results, computed once per scene and never modified


def _graph(name):
    if name not in _G:
        scene, seeds = getattr(sc, name)()
        _G[name] = (scene, seeds, ref.Graphs(scene).graph(seeds, 0, len(seeds[0]) - 1))
    return _G[name]


def _bits(x):
    return np.asarray(x, np.float32).tobytes()


def _fsum(ws):
    s = F32(0)
    for w in ws:
        s = F32(s + w)
    return s


def _edge(g, a, b):
    """Weight of the edge between nodes (view, polyline) a and b, read from the adjacency row of a; None if absent."""
    nodes = list(zip(g["node_view"].tolist(), g["node_pl"].tolist()))
    na, nb = nodes.index(a), nodes.index(b)
    row = slice(int(g["adj_off"][na]), int(g["adj_off"][na + 1]))
    hit = np.nonzero(g["adj_node"][row] == nb)[0]
    return g["adj_w"][row][hit[0]] if len(hit) else None


def test_hand_cases_worked_out():
    """tests/simgraph_cases.py weights_scene. Points 0..5 list, in (view, polyline): 0 {(0,0) (1,0)}; 1 nothing; 2 {(0,0)
    (0,1) (1,0)}; 3 {(0,0) (1,0) (2,2)}; 4 (view 1 twice) {(0,0) (1,0)}; 5 {(0,0) (0,1) (1,0) (1,1) (2,0) (2,1) (2,3)}."""
    scene, seeds, g = _graph("weights_scene")
    assert _bits(g["point_weight"]) == _bits([ONE, 0, W23, ONE, ONE, W37])
    # nodes by first appearance: point 0 brings (0,0) (1,0), point 2 (0,1), point 3 (2,2), point 5 the rest, ascending
    assert list(zip(g["node_view"].tolist(), g["node_pl"].tolist())) == [(0, 0), (1, 0), (0, 1), (2, 2), (1, 1), (2, 0), (2, 1), (2, 3)]
    # close_polylines: the point without a close polyline has an empty row, the doubled view counts once
    assert np.diff(g["cp_off"]).tolist() == [2, 0, 3, 3, 2, 7]
    assert g["cp_view"][int(g["cp_off"][4]):int(g["cp_off"][5])].tolist() == [0, 1]
    # close_refpoints of (0,0): every point but 1, once each
    assert g["cr_point"][int(g["cr_off"][0]):int(g["cr_off"][1])].tolist() == [0, 2, 3, 4, 5]
    # (0,0)-(1,0): A = B = {0, 2, 3, 4, 5}: exactly 1
    assert _bits(_edge(g, (0, 0), (1, 0))) == _bits(ONE)
    # the edge inside view 0, (0,0)-(0,1): A = {0, 2, 3, 4, 5} (all list view 0), B = {2, 5}: the union is larger
    w = F32(_fsum([W23, W37]) / _fsum([ONE, W23, ONE, ONE, W37]))
    assert w < 1 and _bits(_edge(g, (0, 0), (0, 1))) == _bits(w)
    # (0,0)-(2,2): A = the points close to (0,0) that list view 2 = {3, 5}, B = {3}: 1 / (1 + 3/7)
    assert _bits(_edge(g, (0, 0), (2, 2))) == _bits(F32(ONE / F32(ONE + W37)))
    # (1,0)-(1,1): A = {0, 2, 3, 4, 5}, B = {5}
    assert _bits(_edge(g, (1, 0), (1, 1))) == _bits(F32(W37 / _fsum([ONE, W23, ONE, ONE, W37])))
    # point 2 never sees (1,1): no edge between (2,2) and (1,1) (no point lists both)
    assert _edge(g, (2, 2), (1, 1)) is None
    # both directions of every edge, neighbours ascending
    for n in range(g["n_nodes"]):
        row = g["adj_node"][int(g["adj_off"][n]):int(g["adj_off"][n + 1])].tolist()
        assert row == sorted(set(row)) and n not in row
    assert g["n_pair_instances"] == 1 + 0 + 3 + 3 + 1 + 21


def test_sum_order_is_part_of_the_result():
    """order_scene: the union of the edge (0,1)-(1,0) is points 0..3 with weights 1, 2/3, 2/3, 3/7 and the intersection
    points 1..3. Both sums differ in their float bits between ascending and descending order, so a sum in another order is
    caught by this edge."""
    scene, seeds, g = _graph("order_scene")
    assert _bits(g["point_weight"]) == _bits([ONE, W23, W23, W37])
    uni, inter = [ONE, W23, W23, W37], [W23, W23, W37]
    assert _bits(_fsum(uni)) != _bits(_fsum(uni[::-1]))
    assert _bits(_fsum(inter)) != _bits(_fsum(inter[::-1]))
    asc, desc = F32(_fsum(inter) / _fsum(uni)), F32(_fsum(inter[::-1]) / _fsum(uni[::-1]))
    assert _bits(asc) != _bits(desc)
    assert _bits(_edge(g, (0, 1), (1, 0))) == _bits(asc)


def test_rank_key_equals_first_appearance_numbering():
    """Node ids by first appearance through a dict (the reference) against the rank of first[g] << 32 | g (the device), on
    200 random lists of points with random sets of global polyline indices."""
    rng = np.random.default_rng(20181)
    for _ in range(200):
        n_pl = int(rng.integers(1, 40))
        pts = [sorted(set(int(x) for x in rng.integers(0, n_pl, int(rng.integers(0, 7))))) for _ in range(int(rng.integers(1, 30)))]
        node_of = {}
        for gs in pts:
            for g in gs:               # std::set<pair<int, ulong>> iterates (view, polyline) ascending = g ascending
                if g not in node_of:
                    node_of[g] = len(node_of)
        first = {}
        for r, gs in enumerate(pts):
            for g in gs:
                first.setdefault(g, r)
        keys = sorted((first[g] << 32) | g for g in first)
        assert {k & 0xffffffff: i for i, k in enumerate(keys)} == node_of


def _synthetic_graph():
    """A graph whose weights need all 6 significant digits, round up to the next digit, print as 1 and in exponent form."""
    w = np.array([0.123456, 0.1234565, 0.9999995, 0.999999, 1.5e-05, 3.0000001e-10, 0.5, 1.0], np.float32)
    return {"n_nodes": 3, "node_view": np.array([0, 1, 2], np.uint32), "node_pl": np.array([4, 5, 6], np.uint32),
            "adj_off": np.array([0, 3, 6, 8], np.uint32), "adj_node": np.array([1, 2, 2, 0, 2, 2, 0, 1], np.uint32),
            "adj_w": w, "seed_begin": 0, "n_points": 0, "point_weight": np.zeros(0, np.float32),
            "cp_off": np.zeros(1, np.uint32), "cp_view": np.zeros(0, np.uint32), "cp_pl": np.zeros(0, np.uint32),
            "n_polylines": 0, "cr_off": np.zeros(1, np.uint32), "cr_point": np.zeros(0, np.uint32)}


def test_writer_is_the_references_text(tmp_path):
    syn = _synthetic_graph()
    text = ref.graph_text(syn)
    assert "0.123456\n" in text and "0.123457\n" in text and "e-05\n" in text and "e-10\n" in text and " 1\n" in text
    empty = dict(syn, n_nodes=0, adj_off=np.zeros(1, np.uint32), adj_node=np.zeros(0, np.uint32), adj_w=np.zeros(0, np.float32))
    for name, g in (("syn", syn), ("empty", empty), ("weights", _graph("weights_scene")[2]), ("order", _graph("order_scene")[2])):
        path = str(tmp_path / (name + ".txt"))
        host.write_compat_graph(path, g)
        assert open(path, "rb").read() == ref.graph_text(g).encode(), name
    assert ref.graph_text(empty) == "p sp 0 0\n"
    with pytest.raises(RuntimeError):
        host.write_compat_graph(str(tmp_path / "no_such_dir" / "g.txt"), syn)


def test_communities_to_sets(tmp_path):
    """Community ids with a negative id (the node is dropped), a skipped id (an empty set) and repeats, through the file
    reader and the set builder, against the restatement; the sets pass eg3d_check_polyline_sets."""
    scene, seeds, g = _graph("weights_scene")
    ids = [2, 2, 0, -1, 0, 4, 4, 2]          # community 1 and 3: no node; node 3 dropped
    path = str(tmp_path / "communities.txt")
    open(path, "w").write("".join("%d\n" % i for i in ids))
    got_ids = host.read_communities(path)
    assert got_ids.dtype == np.int64 and got_ids.tolist() == ids
    n_sets, row_off, pl_ids = host.sets_from_communities(g, got_ids, scene["n_views"])
    want = ref.sets_from_communities(g, ids, scene["n_views"])
    assert n_sets == want[0] == 5
    assert row_off.dtype == np.uint32 and np.array_equal(row_off, want[1]) and np.array_equal(pl_ids, want[2])
    V = scene["n_views"]
    assert row_off[1 * V] == row_off[2 * V] and row_off[3 * V] == row_off[4 * V]      # the skipped ids: empty sets
    api.check_polyline_sets(n_sets, row_off, pl_ids, V)
    # every id negative: no set at all
    n0, r0, p0 = host.sets_from_communities(g, [-1] * g["n_nodes"], V)
    assert n0 == 0 and r0.tolist() == [0] and len(p0) == 0
    # a wrong number of ids is refused
    for bad in (ids[:-1], ids + [0]):
        with pytest.raises(RuntimeError):
            host.sets_from_communities(g, bad, V)
    # a line that is no number is refused; a missing file too
    open(path, "w").write("1\nx\n")
    with pytest.raises(RuntimeError):
        host.read_communities(path)
    with pytest.raises(RuntimeError):
        host.read_communities(str(tmp_path / "missing.txt"))


def test_abi_small_struct_size_is_refused_before_anything_else():
    st = D.SimgraphStats()
    st.struct_size = C.sizeof(D.SimgraphStats) - 4
    g = D.Simgraph()
    assert api.lib().eg3d_similarity_graph(None, None, 0, 0, C.byref(g), C.byref(st)) == -1
    assert b"struct_size" in api.lib().eg3d_last_error()
