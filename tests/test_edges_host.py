"""The sequential statement of the 3-D edge model (eg3d_host_edge_chains, include/eg3d/host_edges.h) against the independent
numpy restatement tests/edges_ref.py, array for array and bit for bit: the enumerated graphs of tests/edges_cases.py, the host
replay graph of C2 built from the oracle's cloud, 40 seeded random graphs; the refusals; the PLY writer. No GPU."""
import os

import numpy as np
import pytest

import edges_cases as ec
import edges_ref as er
from edgegraph3d_amd import host
from oracle import binding as ob

CASES = ec.cases()
RANDOM = ec.random_cases()


def _held(name, g, max_dist):
    for on in (True, False):
        got = host.edge_chains(g, max_dist, simplify=on)
        want = er.edge_chains(g, max_dist, simplify_on=on)
        assert er.difference(got, want) is None, (name, on, er.difference(got, want))
    return got, want


@pytest.mark.parametrize("name", sorted(CASES))
def test_enumerated_graph(name):
    g, max_dist = CASES[name]
    _held(name, g, max_dist)


def test_the_cases_are_what_their_names_say():
    """What each group is there for, read from the restatement's result (so a case that stopped exercising its rule shows)."""
    def ref(name, **kw):
        g, d = CASES[name]
        return er.edge_chains(g, d, **kw)
    assert ref("empty")["stats"]["n_chains"] == 0 and ref("nodes_without_polylines")["stats"]["n_chains"] == 0
    assert ref("one_polyline")["chain_node"].tolist() == [1, 0]
    assert ref("path_reversed_orientation")["chain_node"].tolist() == [2, 1, 0]
    assert ref("path_reversed_orientation_b")["chain_node"].tolist() == [2, 1, 0]
    star = ref("star_1_2_5")
    assert sorted(np.diff(star["chain_off"]).tolist()) == [2, 3, 6] and star["stats"]["n_rings"] == 0
    for n in (3, 64, 65):
        r = ref("ring_%d" % n)
        assert r["flags"].tolist() == [1] and r["chain_node"][0] == r["chain_node"][-1] == 0 and len(r["chain_node"]) == n + 1
    r = ref("ring_smallest_node_off_polyline_0")
    assert r["chain_node"].tolist() == [0, 1, 2, 3, 0]          # leaves node 0 along polyline 1, not 2
    for name in ("closed_chain_on_a_hub", "closed_chain_on_a_hub_reversed"):
        r = ref(name)
        assert r["flags"].tolist() == [0, 0] and r["stats"]["n_rings"] == 0
        closed = [r["chain_node"][int(a):int(b)].tolist() for a, b in zip(r["chain_off"][:-1], r["chain_off"][1:]) if b - a == 5]
        assert len(closed) == 1 and closed[0][0] == closed[0][-1] == 0
        kept = [r["s_node"][int(a):int(b)].tolist() for a, b in zip(r["s_off"][:-1], r["s_off"][1:])]
        assert [0, 1, 2, 3, 0] in kept or [0, 3, 2, 1, 0] in kept   # E1: the square keeps its corners
    r = ref("loop_on_a_pass_through_node")
    assert r["chain_node"].tolist() == [0, 1, 2] and r["stats"]["n_loops_dropped"] == 1
    r = ref("loop_on_an_isolated_node")
    assert r["chain_node"].tolist() == [0, 1] and r["stats"]["n_loops_dropped"] == 1
    for n in (63, 64, 65, 1025):
        r = ref("path_%d_shuffled" % n)
        assert r["stats"]["n_chains"] == 1 and r["stats"]["longest_chain"] == n + 1 and r["stats"]["n_vertices_kept"] == 8
    r = ref("two_chains_interleaved")
    assert r["chain_node"].tolist() == [4, 5, 6, 7, 0, 1, 2, 3]
    assert ref("two_vertices")["s_node"].tolist() == [0, 1] and ref("three_vertices")["s_node"].tolist() == [0, 1, 2]
    assert ref("collinear")["s_node"].tolist() == [0, 4] and ref("an_L")["s_node"].tolist() == [0, 2, 4]
    assert ref("zigzag")["s_node"].tolist() == list(range(9))
    assert ref("quotient_equals_maxsq")["s_node"].tolist() == [0, 2]
    assert ref("quotient_just_above_maxsq")["s_node"].tolist() == [0, 1, 2]
    d = er.distance_point_line_sq(np.float32([1, 0.5, 0]), np.float32([0, 0, 0]), np.float32([4, 0, 0]))
    assert d[0] == np.float32(0.25) == np.float32(0.5) * np.float32(0.5)
    info = {}
    ref("first_eb_before_se", info=info)
    assert info["rounds"] >= 2
    for n in (65, 129):
        r = ref("arc_%d" % n)
        assert 2 < r["stats"]["n_vertices_kept"] < n
    assert ref("max_dist_zero_zigzag")["s_node"].tolist() == list(range(9))
    assert ref("max_dist_zero_collinear")["s_node"].tolist() == [0, 4]
    assert ref("max_dist_huge")["s_node"].tolist() == [0, 8]
    r = ref("ring_simplified")
    assert r["s_node"][0] == r["s_node"][-1] == 0 and 3 < len(r["s_node"]) < 66


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_random_graph(name):
    g, max_dist = RANDOM[name]
    _held(name, g, max_dist)


def test_random_graphs_cover_the_kinds():
    st = [er.edge_chains(g, d)["stats"] for g, d in RANDOM.values()]
    assert sum(s["n_rings"] for s in st) > 0 and sum(s["n_loops_dropped"] for s in st) > 0
    assert max(s["longest_chain"] for s in st) > 10 and any(s["n_vertices_kept"] < s["n_vertices_in"] for s in st)
    assert all(int(g["n_nodes"]) <= 200 for g, _ in RANDOM.values())


def test_the_replay_graph_of_c2():
    s = host.Synth(2)
    cloud = ob.Oracle(s.scene).match(s.seeds, 0, s.n_seeds, min(16, os.cpu_count() or 1))
    g = host.replay_matches(s.scene, cloud)
    assert g["n_polylines"] > 1000
    got = host.edge_chains(g, 0.05)
    want = er.edge_chains(g, 0.05)
    assert er.difference(got, want) is None, er.difference(got, want)
    st = got["stats"]
    print("C2: %d nodes, %d polylines -> %d chains (%d rings, %d loops), longest %d, %d vertices -> %d kept at 0.05"
          % (g["n_nodes"], g["n_polylines"], st["n_chains"], st["n_rings"], st["n_loops_dropped"], st["longest_chain"],
             st["n_vertices_in"], st["n_vertices_kept"]))
    assert st["n_chains"] > 0 and st["longest_chain"] > 2 and st["n_vertices_kept"] < st["n_vertices_in"]
    # unsimplified: the trace of the restatement above, every vertex kept, the length over all of them
    plain = host.edge_chains(g, 0.05, simplify=False)
    for k in ("chain_off", "chain_node", "flags"):
        assert plain[k].tobytes() == want[k].tobytes(), k
    assert plain["s_off"].tobytes() == want["chain_off"].tobytes() and plain["s_node"].tobytes() == want["chain_node"].tobytes()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _refused(g, max_dist):
    """-1, and the output struct untouched: the call is made through ctypes with a marked struct."""
    import ctypes as C
    from edgegraph3d_amd import _cdefs as D
    ga = D.EdgesGraphArrays(g)
    ch, st = D.EdgeChains(), D.EdgesStats()
    C.memset(C.byref(ch), 0xA5, C.sizeof(ch))
    st.struct_size, st.n_chains = C.sizeof(D.EdgesStats), 0x1234
    before = bytes(ch)
    rc = host.lib().eg3d_host_edge_chains(C.byref(ga.c), C.c_float(max_dist), 1, C.byref(ch), C.byref(st))
    assert rc == -1, rc
    assert bytes(ch) == before and st.n_chains == 0x1234
    with pytest.raises(ValueError) as e:
        host.edge_chains(g, max_dist)
    assert e.value.code == -1


@pytest.mark.parametrize("name", sorted(ec.broken_graphs()))
def test_inconsistent_graph_is_refused(name):
    _refused(ec.broken_graphs()[name], 0.01)


@pytest.mark.parametrize("max_dist", [float("nan"), -0.01, float("inf"), float("-inf")], ids=["nan", "negative", "inf", "-inf"])
def test_bad_max_dist_is_refused(max_dist):
    _refused(CASES["an_L"][0], max_dist)


def test_sound_base_graph_and_small_stats_struct():
    import ctypes as C
    from edgegraph3d_amd import _cdefs as D
    g = ec.make_graph(4, [(0, 1), (1, 2), (2, 2), (2, 3)])
    assert host.edge_chains(g, 0.01)["stats"]["n_loops_dropped"] == 1     # what broken_graphs() breaks is sound
    ga, ch, st = D.EdgesGraphArrays(g), D.EdgeChains(), D.EdgesStats()
    st.struct_size = C.sizeof(D.EdgesStats) - 4
    assert host.lib().eg3d_host_edge_chains(C.byref(ga.c), 0.01, 1, C.byref(ch), C.byref(st)) == -1
    assert host.lib().eg3d_host_edge_chains(None, 0.01, 1, C.byref(ch), None) == -1
    assert host.lib().eg3d_host_edge_chains(C.byref(ga.c), 0.01, 1, None, None) == -1
    with pytest.raises(ValueError):
        bad = dict(g)
        bad["pl_end"] = g["pl_end"][:-1]
        host.edge_chains(bad, 0.01)


# ---- the writer ----------------------------------------------------------------------------------------------------------------
def test_ply_edges_byte_for_byte(tmp_path):
    """Two chains: 5 - 3 - 1 (node ids out of order, a float that %g shortens, one it writes with an exponent) and 1 - 6."""
    X = np.zeros((7, 3), np.float32)
    X[1], X[3], X[5], X[6] = [0.5, -2, 1e-7], [1.25, 0, 3], [0.1, 100000, 1234567], [-1, -1, -1]
    chains = {"chain_off": [0, 3, 5], "chain_node": [5, 3, 1, 1, 6], "flags": [0, 0], "s_off": [0, 3, 5],
              "s_node": [5, 3, 1, 1, 6], "length": [0, 0]}
    path = tmp_path / "edges.ply"
    host.write_ply_edges(str(path), chains, X)
    want = ("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
            "element edge 3\nproperty int vertex1\nproperty int vertex2\nend_header\n"
            "0.5 -2 1e-07\n1.25 0 3\n0.1 100000 1.23457e+06\n-1 -1 -1\n"
            "2 1\n1 0\n0 3\n")
    assert path.read_bytes() == want.encode()
    # an empty model is a header alone; a node id outside node_X is refused before the library sees it
    host.write_ply_edges(str(path), {"chain_off": [0], "chain_node": [], "flags": [], "s_off": [0], "s_node": [], "length": []}, X)
    assert path.read_bytes().endswith(b"element vertex 0\nproperty float x\nproperty float y\nproperty float z\nelement edge 0\n"
                                      b"property int vertex1\nproperty int vertex2\nend_header\n")
    with pytest.raises(ValueError):
        host.write_ply_edges(str(path), chains, X[:6])
    with pytest.raises(OSError):
        host.write_ply_edges(str(tmp_path / "no_such_dir" / "e.ply"), chains, X)
