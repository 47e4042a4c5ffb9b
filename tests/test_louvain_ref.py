"""CPU: the restatement of K11 (tests/louvain_ref.py, the definition of eg3d_detect_communities) on hand graphs and against
checks that do not share its code; the library side that needs no device (refusals, the communities file; symbols and
struct mirrors: tests/test_abi.py). The planted partitions use seeds 0-4 of louvain_ref.planted: all five recover the blocks exactly."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import louvain_ref as L
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host

_RUNS = {}   # per graph name: (graph, result), computed once and never modified


def _run(name, make):
    if name not in _RUNS:
        g = make()
        _RUNS[name] = (g, L.louvain(*g))
    return _RUNS[name]


# ---- library checks ------------------------------------------------------------------------------------------------------------
def test_null_context_and_small_structs_are_refused():
    lib = api.lib()
    n, off, node, w = L.two_triangles()
    sg = D.Simgraph()
    sg.n_nodes, sg.adj_off, sg.adj_node, sg.adj_w = n, D.np_ptr(off, C.c_uint32), D.np_ptr(node, C.c_uint32), D.np_ptr(w, C.c_float)
    m, st = D.Communities(), D.LouvainStats()
    st.struct_size = C.sizeof(D.LouvainStats)
    assert lib.eg3d_detect_communities(None, C.byref(sg), None, C.byref(m), C.byref(st)) == -1
    assert b"bad arguments" in lib.eg3d_last_error()
    assert not m.ids and m.n_nodes == 0 and st.n_sweeps == 0
    st.struct_size -= 4
    assert lib.eg3d_detect_communities(None, C.byref(sg), None, C.byref(m), C.byref(st)) == -1
    assert b"stats->struct_size" in lib.eg3d_last_error()
    st.struct_size = C.sizeof(D.LouvainStats)
    pr = D.LouvainParams(C.sizeof(D.LouvainParams) - 4)
    assert lib.eg3d_detect_communities(None, C.byref(sg), C.byref(pr), C.byref(m), C.byref(st)) == -1
    assert b"params->struct_size" in lib.eg3d_last_error()
    lib.eg3d_free_communities(C.byref(m))      # (an empty result may be freed)
    lib.eg3d_free_communities(None)


# ---- the restatement on hand graphs ------------------------------------------------------------------------------------------
def test_two_triangles_with_a_bridge_and_an_isolated_node():
    _, r = _run("two_triangles", L.two_triangles)
    assert r["ids"].tolist() == [0, 0, 0, 1, 1, 1, -1]
    assert r["n_communities"] == 2 and r["n_isolated"] == 1


def test_k6_is_one_community():
    _, r = _run("k6", L.clique)
    assert r["ids"].tolist() == [0] * 6 and r["n_communities"] == 1 and r["numer"] == 0


def test_star_of_200_leaves_is_one_community():
    _, r = _run("star", L.star)
    assert r["ids"].tolist() == [0] * 201 and r["n_communities"] == 1


def test_ring_of_30_five_cliques():
    _, r = _run("ring", L.ring_of_cliques)
    assert r["ids"].tolist() == [i // 5 for i in range(150)] and r["n_communities"] == 30


@pytest.mark.parametrize("seed", range(5))
def test_planted_partition_is_recovered_exactly(seed):
    _, r = _run("planted%d" % seed, lambda: L.planted(seed))
    assert r["ids"].tolist() == [i // 24 for i in range(192)]
    assert 2 <= r["n_phases"] <= 3 and 9 <= r["n_sweeps"] <= 16 and 0.83 < r["modularity"] < 0.86


def test_path_of_100_nodes():
    _, r = _run("path", L.path)
    assert (r["n_communities"], r["n_phases"], r["n_sweeps"]) == (12, 4, 89)
    ids = r["ids"].tolist()
    assert ids == sorted(ids)      # (every community is a stretch of the path)


# ---- checks that do not share the restatement's code ----------------------------------------------------------------------------
def _textbook_modularity(g, ids):
    """Q = sum over communities of in_c / 2m - (tot_c / 2m)^2, from the original graph, in exact fractions."""
    n, off, node, w = g
    q = [L.quantize(x) for x in w]
    two_m = sum(q)
    inside, tot = {}, {}
    for i in range(n):
        for p in range(int(off[i]), int(off[i + 1])):
            tot[ids[i]] = tot.get(ids[i], 0) + q[p]
            if ids[i] == ids[int(node[p])]:
                inside[ids[i]] = inside.get(ids[i], 0) + q[p]
    return sum(Fraction(inside.get(c, 0), two_m) - Fraction(tot[c], two_m) ** 2 for c in tot)


HAND = {"two_triangles": L.two_triangles, "k6": L.clique, "star": L.star, "ring": L.ring_of_cliques, "path": L.path,
        "planted0": lambda: L.planted(0), "planted1": lambda: L.planted(1), "long_row": L.long_row}


@pytest.mark.parametrize("name", sorted(HAND))
def test_properties(name):
    g, r = _run(name, HAND[name])
    M, N, ids = r["total_q"], r["numer"], r["ids"].tolist()
    # the modularity of the final ids, recomputed from the textbook formula on the original graph, is N / M^2 exactly
    assert _textbook_modularity(g, ids) == Fraction(N, M * M)
    assert r["modularity"] == float(N) / (float(M) * float(M))
    assert (r["numer_hi"] << 64 | r["numer_lo"]) == N % 2 ** 128
    # every accepted sweep raises N; coarsening preserves it: N0 of a phase is the final N of the phase before
    for ph in r["trace"]:
        assert all(b > a for a, b in zip(ph, ph[1:]))
    for a, b in zip(r["trace"], r["trace"][1:]):
        assert b[0] == a[-1]
    assert r["trace"][-1][-1] == N
    # ids are numbered by ascending smallest member; nodes without a row are -1
    first = {}
    for i, c in enumerate(ids):
        if c >= 0:
            first.setdefault(c, i)
    assert [first[c] for c in sorted(first)] == sorted(first.values()) and sorted(first) == list(range(r["n_communities"]))
    assert r["n_isolated"] == ids.count(-1)


def test_a_single_edge_stays_together():
    """Both ends would move to the other's community in the first sweep; swap protection keeps the smaller label in place, so
    node 1 joins node 0 instead of the two trading places for ever."""
    r = L.louvain(2, *L.csr_from_edges(2, [(0, 1, 0.5)]))
    assert r["ids"].tolist() == [0, 0] and (r["n_phases"], r["n_sweeps"]) == (2, 3)   # (2 sweeps, then 1 on the single coarse vertex)
    rows, k = [[(1, 5)], [(0, 5)]], [5, 5]
    assert [L.target(i, rows, [0, 1], k, [5, 5], [1, 1], 10) for i in (0, 1)] == [0, 0]


def test_equal_gains_go_to_the_smaller_label():
    """An equal-weight 4-cycle: node 0 gains the same from joining 1 or 3 and takes 1; node 2 likewise; swap protection then
    holds 0 (1 > 0 is refused for the smaller label) while 1, 2, 3 move to the smaller of their two equal choices."""
    n, off, node, w = (4,) + L.csr_from_edges(4, [(0, 1, 0.5), (1, 2, 0.5), (2, 3, 0.5), (0, 3, 0.5)])
    rows = [[(int(node[p]), L.quantize(w[p])) for p in range(int(off[i]), int(off[i + 1]))] for i in range(4)]
    k = [sum(q for _, q in r) for r in rows]
    M = sum(k)
    T = [L.target(i, rows, [0, 1, 2, 3], k, list(k), [1] * 4, M) for i in range(4)]
    assert T == [0, 0, 1, 0]
    # without swap protection node 0 would have taken 1, the smaller of the equal labels 1 and 3
    assert L.target(0, rows, [0, 1, 2, 3], k, list(k), [2, 1, 1, 1], M) == 1


def test_weights_at_the_ends_of_the_range():
    assert L.quantize(1.0) == 2 ** 32 and L.quantize(np.float32(2.0 ** -34)) == 0 and L.quantize(np.float32(2.0 ** -33)) == 0
    assert L.quantize(np.float32(1.5 * 2.0 ** -32)) == 2      # ties go to even, as llrint
    assert L.quantize(np.float32(0.1)) == 429496736            # 0.1f = 13421773 * 2^-27: the product with 2^32 is an integer
    # an entry with q == 0 stays in the graph with weight 0: it keeps its node live (an id, not -1) and attracts nothing
    tiny = np.float32(2.0 ** -40)
    r = L.louvain(5, *L.csr_from_edges(5, [(0, 1, 1.0), (1, 2, 1.0), (0, 2, 1.0), (2, 3, tiny)]))
    assert r["ids"].tolist() == [0, 0, 0, 1, -1] and r["total_q"] == 6 * 2 ** 32
    # no weight at all: every node with a row alone, numbered in order, nothing swept
    r = L.louvain(4, *L.csr_from_edges(4, [(1, 3, tiny)]))
    assert r["ids"].tolist() == [-1, 0, -1, 1] and (r["n_phases"], r["n_sweeps"], r["total_q"], r["modularity"]) == (0, 0, 0, 0.0)
    # w == 1.0 everywhere: K6's degrees are 5 * 2^32 and M is 30 * 2^32
    assert _run("k6", L.clique)[1]["total_q"] == 30 * 2 ** 32


def test_parameters():
    g = L.planted(0)
    one = L.louvain(*g, max_sweeps=1)
    assert one["n_sweeps"] == one["n_phases"]
    assert L.louvain(*g, max_phases=1)["n_phases"] == 1
    assert L.louvain(*g)["ids"].tolist() == L.louvain(*g, max_phases=200, max_sweeps=1000, sweep_threshold=1e-6,
                                                      phase_threshold=1e-6)["ids"].tolist()


# ---- the communities file ------------------------------------------------------------------------------------------------------
def test_communities_file_round_trip(tmp_path):
    path = str(tmp_path / "communities.txt")
    ids = np.array([0, 0, -1, 1, 2 ** 40, -1, 3], np.int64)
    host.write_communities(path, ids)
    assert open(path).read() == L.communities_text(ids) == "0\n0\n-1\n1\n1099511627776\n-1\n3\n"
    back = host.read_communities(path)
    assert back.dtype == np.int64 and back.tolist() == ids.tolist()
    host.write_communities(path, [])
    assert open(path).read() == "" and len(host.read_communities(path)) == 0
    with pytest.raises(RuntimeError):
        host.write_communities(str(tmp_path / "no_such_dir" / "c.txt"), ids)
