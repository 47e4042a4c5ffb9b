"""-m gpu: eg3d_detect_communities (K11) against its definition, the Python restatement tests/louvain_ref.py, on the same CSR.
ids are compared byte for byte; n_phases, n_sweeps, n_communities, total_q and the 128-bit numerator must be equal and the
modularity must have the same bits. Every graph runs with the default table and with EG3D_LOUVAIN_TABLE_SLOTS=16, which sends
every row with more than 16 distinct neighbouring communities through the sort-and-reduce path."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import cbuild
import louvain_ref as L
import polymatch_ref as pref
import simgraph_ref as sref
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host
from oracle import binding as ob
from parity_util import compare_edgepoints

pytestmark = pytest.mark.gpu

GRAPHS = {
    "two_triangles": L.two_triangles, "k6": L.clique, "star200": L.star, "ring": L.ring_of_cliques, "path100": L.path,
    "planted192": lambda: L.planted(0), "planted192_s1": lambda: L.planted(1), "planted192_s2": lambda: L.planted(2),
    "planted192_s3": lambda: L.planted(3), "planted192_s4": lambda: L.planted(4),
    "planted2000": lambda: L.planted(7, blocks=40, size=50, p_in=0.35, p_out=0.0005),
    "row1500": L.long_row,
}
_REF = {}    # per graph (and parameters): (graph dict, the restatement's result), computed once and never modified
_CTX = {}    # per table size: a context on synthetic config 0 (the scene plays no part in K11; a context needs one)
_SYNTH = {}


def _synth(cfg):
    if cfg not in _SYNTH:
        s = host.Synth(cfg)
        _SYNTH[cfg] = (s, s.scene_np(), s.seeds_np())
    return _SYNTH[cfg]


def _context(slots=None, scene=None):
    """A fresh context; EG3D_LOUVAIN_TABLE_SLOTS is read when a context is created."""
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    old = os.environ.pop("EG3D_LOUVAIN_TABLE_SLOTS", None)
    try:
        if slots is not None:
            os.environ["EG3D_LOUVAIN_TABLE_SLOTS"] = str(slots)
        return api.Context(scene if scene is not None else _synth(0)[0].scene)
    finally:
        os.environ.pop("EG3D_LOUVAIN_TABLE_SLOTS", None)
        if old is not None:
            os.environ["EG3D_LOUVAIN_TABLE_SLOTS"] = old


def _ctx(slots=None):
    if slots not in _CTX:
        _CTX[slots] = _context(slots)
    return _CTX[slots]


def teardown_module(module):
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def _graph(name):
    n, off, node, w = GRAPHS[name]()
    return {"n_nodes": n, "adj_off": off, "adj_node": node, "adj_w": w}


def _want(name, **params):
    key = (name,) + tuple(sorted(params.items()))
    if key not in _REF:
        g = _REF[(name,)][0] if (name,) in _REF else _graph(name)
        _REF[key] = (g, L.louvain(g["n_nodes"], g["adj_off"], g["adj_node"], g["adj_w"], **params))
    return _REF[key]


def _bits(x):
    return struct.pack("<d", x)


def _same(got, want):
    st = got["stats"]
    print("got: communities %d phases %d sweeps %d M %d N %d Q %r overflow rows %d | want: %d %d %d %d %d %r" % (
        got["n_communities"], st["n_phases"], st["n_sweeps"], st["total_q"], st["numer_hi"] << 64 | st["numer_lo"], st["modularity"],
        st["n_overflow_rows"], want["n_communities"], want["n_phases"], want["n_sweeps"], want["total_q"],
        want["numer_hi"] << 64 | want["numer_lo"], want["modularity"]))
    assert got["ids"].dtype == np.int64 and got["ids"].tobytes() == want["ids"].tobytes(), (got["ids"], want["ids"])
    assert got["n_communities"] == want["n_communities"]
    for k in ("n_phases", "n_sweeps", "n_communities", "n_isolated", "total_q", "numer_hi", "numer_lo"):
        assert st[k] == want[k], (k, st[k], want[k])
    assert _bits(st["modularity"]) == _bits(want["modularity"])


def _max_row(g):
    return int(np.diff(g["adj_off"].astype(np.int64)).max()) if g["n_nodes"] else 0


@pytest.mark.parametrize("name", list(GRAPHS))
def test_hand_graphs(name):
    """The hand graphs of the CPU test, the 100-node path, planted graphs of 192 and 2 000 nodes, the star whose centre row
    crosses a wavefront (200 entries) and a row of 1 500 entries: the default table, then 16 slots."""
    g, want = _want(name)
    got = _ctx().communities(g)
    _same(got, want)
    if _max_row(g) <= 512:
        assert got["stats"]["n_overflow_rows"] == 0
    else:
        assert got["stats"]["n_overflow_rows"] > 0         # (row1500: its first sweep sees 1 500 communities)
    small = _ctx(16).communities(g)
    _same(small, want)
    if _max_row(g) > 16:                                    # the first sweep: every neighbour is a community of its own
        assert small["stats"]["n_overflow_rows"] > 0
    else:
        assert small["stats"]["n_overflow_rows"] == 0


def test_the_graphs_reach_both_paths():
    """What the shapes are for, checked on the inputs: rows on both sides of 16 and of 64, one beyond the largest table."""
    rows = {n: _max_row(_want(n)[0]) for n in GRAPHS}
    assert rows["two_triangles"] <= 16 and rows["path100"] == 2 and 16 < rows["planted192"] < 64
    assert rows["star200"] == 200 and rows["row1500"] == 1500 and rows["planted2000"] > 16


@pytest.mark.parametrize("params", [{"max_sweeps": 1}, {"max_phases": 1}, {"max_sweeps": 2, "max_phases": 2},
                                    {"sweep_threshold": 1e-2}, {"phase_threshold": 0.5}],
                         ids=["max_sweeps1", "max_phases1", "two_and_two", "sweep_threshold", "phase_threshold"])
def test_parameters(params):
    for name in ("planted192", "path100"):
        g, want = _want(name, **params)
        _same(_ctx().communities(g, **params), want)
        _same(_ctx(16).communities(g, **params), want)
    assert _want("planted192", max_phases=1)[1]["n_phases"] == 1
    one = _want("planted192", max_sweeps=1)[1]
    assert one["n_sweeps"] == one["n_phases"]
    with pytest.raises(api.Eg3dError):
        _ctx().communities(_want("k6")[0], sweep_threshold=-1.0)


def test_determinism_and_clone():
    g, want = _want("planted2000")
    ctx = _ctx()
    a, b = ctx.communities(g), ctx.communities(g)
    clone = ctx.clone()
    c = clone.communities(g)
    clone.close()
    for r in (a, b, c):
        _same(r, want)
    assert a["ids"].tobytes() == b["ids"].tobytes() == c["ids"].tobytes()
    small = _ctx(16)
    clone = small.clone()                       # (a clone keeps the table size of its parent)
    d = clone.communities(g)
    clone.close()
    _same(d, want)
    assert d["stats"]["n_overflow_rows"] > 0


def _bad(kind):
    n, off, node, w = [a.copy() if hasattr(a, "copy") else a for a in L.two_triangles()]
    # rows: 0 [1 2]  1 [0 2]  2 [0 1 3]  3 [2 4 5]  4 [3 5]  5 [3 4]  6 []
    rev01 = int(off[1])                          # the entry 1 -> 0
    if kind == "asymmetric":
        node[1] = 4                              # 0 -> 4 has no 4 -> 0
    elif kind == "weight_bits":
        w[0] = np.nextafter(w[0], np.float32(0))
    elif kind == "unsorted":
        node[0], node[1] = 2, 1
    elif kind == "self_loop":
        node[0] = 0
    elif kind == "w_above_1":
        w[0] = w[rev01] = 1.5
    elif kind == "w_zero":
        w[0] = w[rev01] = 0.0
    elif kind == "w_nan":
        w[0] = w[rev01] = np.nan
    elif kind == "w_inf":
        w[0] = w[rev01] = np.inf
    elif kind == "neighbour_range":
        node[0] = 7
    elif kind == "offsets":
        off[1], off[2] = 4, 2
    return {"n_nodes": n, "adj_off": off, "adj_node": node, "adj_w": w}


REFUSALS = {"asymmetric": b"no reverse entry", "weight_bits": b"different weight bits", "unsorted": b"not strictly ascending",
            "self_loop": b"self-loop", "w_above_1": b"in (0, 1]", "w_zero": b"in (0, 1]", "w_nan": b"in (0, 1]",
            "w_inf": b"in (0, 1]", "neighbour_range": b"not below n_nodes", "offsets": b"adj_off"}


@pytest.mark.parametrize("kind", list(REFUSALS))
@pytest.mark.parametrize("slots", [None, 16], ids=["default", "slots16"])
def test_refusals(kind, slots):
    """Every rule of the input: EG3D_ERR_ARG with a message that names it, the outputs untouched, and the next valid call on
    the same context is correct."""
    ctx = _ctx(slots)
    g = _bad(kind)
    sg = D.Simgraph()
    sg.n_nodes = g["n_nodes"]
    sg.adj_off, sg.adj_node, sg.adj_w = (D.np_ptr(g["adj_off"], C.c_uint32), D.np_ptr(g["adj_node"], C.c_uint32),
                                         D.np_ptr(g["adj_w"], C.c_float))
    m, st = D.Communities(), D.LouvainStats()
    st.struct_size = C.sizeof(D.LouvainStats)
    rc = api.lib().eg3d_detect_communities(ctx._h, C.byref(sg), None, C.byref(m), C.byref(st))
    err = api.lib().eg3d_last_error()
    assert rc == -1 and REFUSALS[kind] in err, (rc, err)
    assert not m.ids and m.n_nodes == 0 and m.n_communities == 0
    assert (st.n_phases, st.n_sweeps, st.n_communities, st.total_q, st.numer_lo, st.modularity) == (0, 0, 0, 0, 0, 0.0)
    with pytest.raises(api.Eg3dError):
        ctx.communities(g)
    g, want = _want("two_triangles")
    _same(ctx.communities(g), want)


def test_empty_graphs():
    ctx = _ctx()
    none = ctx.communities({"n_nodes": 0, "adj_off": np.zeros(1, np.uint32), "adj_node": np.zeros(0, np.uint32),
                            "adj_w": np.zeros(0, np.float32)})
    assert len(none["ids"]) == 0 and none["n_communities"] == 0 and none["stats"]["n_sweeps"] == 0
    g = {"n_nodes": 5, "adj_off": np.zeros(6, np.uint32), "adj_node": np.zeros(0, np.uint32), "adj_w": np.zeros(0, np.float32)}
    want = L.louvain(5, g["adj_off"], g["adj_node"], g["adj_w"])
    got = ctx.communities(g)
    _same(got, want)
    assert got["ids"].tolist() == [-1] * 5 and got["stats"]["n_isolated"] == 5
    # weights that all quantize to 0: every node with a row alone, numbered in order, nothing swept
    tiny = np.float32(2.0 ** -40)
    n, off, node, w = (4,) + L.csr_from_edges(4, [(1, 3, tiny)])
    g = {"n_nodes": n, "adj_off": off, "adj_node": node, "adj_w": w}
    got = ctx.communities(g)
    _same(got, L.louvain(n, off, node, w))
    assert got["ids"].tolist() == [-1, 0, -1, 1] and got["stats"]["n_phases"] == 0
    # a q == 0 entry beside real weights, and w == 1.0
    n, off, node, w = (5,) + L.csr_from_edges(5, [(0, 1, 1.0), (1, 2, 1.0), (0, 2, 1.0), (2, 3, tiny)])
    g = {"n_nodes": n, "adj_off": off, "adj_node": node, "adj_w": w}
    got = ctx.communities(g)
    _same(got, L.louvain(n, off, node, w))
    assert got["ids"].tolist() == [0, 0, 0, 1, -1]


# ---- behind eg3d_similarity_graph ------------------------------------------------------------------------------------------------
def _simgraph_want(cfg, b, e):
    key = ("simgraph", cfg, b, e)
    if key not in _REF:
        _, scene, seeds = _synth(cfg)
        m = pref.Matcher(scene)
        g = sref.similarity_graph(scene, m.entry_results(seeds, b, e))
        _REF[key] = (g, L.louvain(g["n_nodes"], g["adj_off"], g["adj_node"], g["adj_w"]))
    return _REF[key]


@pytest.mark.parametrize("cfg,n_seeds", [(0, None), (2, 2000)], ids=["config0", "config2_first_2000"])
def test_pipeline(cfg, n_seeds):
    """ctx.communities(ctx.similarity_graph(...)) equals the restatement run on tests/simgraph_ref.py's graph."""
    s = _synth(cfg)[0]
    n = s.n_seeds if n_seeds is None else n_seeds
    assert s.n_seeds >= n
    g_want, want = _simgraph_want(cfg, 0, n)
    for slots in (None, 16):
        ctx = _context(slots, s.scene)
        ctx.upload_seeds(s.seeds)
        g = ctx.similarity_graph(None, 0, n)
        assert g["adj_off"].tobytes() == g_want["adj_off"].tobytes() and g["adj_w"].tobytes() == g_want["adj_w"].tobytes()
        _same(ctx.communities(g), want)
        ctx.close()
    if cfg == 2:
        assert g_want["n_nodes"] > 500 and want["n_communities"] > 1


def test_end_to_end_without_a_file():
    """Config 0: the sets built from K11's ids go into eg3d_match_polyline_sets, and the cloud equals the oracle's extractor on
    the sets built from the restatement's ids."""
    s, scene, _ = _synth(0)
    V = scene["n_views"]
    g_want, want = _simgraph_want(0, 0, s.n_seeds)
    ctx = _context(None, s.scene)
    g = ctx.similarity_graph(s.seeds)
    got = ctx.communities(g)
    _same(got, want)
    n_sets, row_off, pl_ids = host.sets_from_communities(g, got["ids"], V)
    w_sets, w_off, w_ids = sref.sets_from_communities(g_want, want["ids"], V)
    assert n_sets == w_sets == want["n_communities"] and np.array_equal(row_off, w_off) and np.array_equal(pl_ids, w_ids)
    api.check_polyline_sets(n_sets, row_off, pl_ids, V)
    cloud = ctx.match_polyline_sets(n_sets, row_off, pl_ids)
    orc = ob.Oracle(s.scene).match_polyline_sets(w_sets, w_off, w_ids)
    rep = compare_edgepoints(orc, cloud)
    assert rep["ok"], rep["msgs"]
    assert cloud["n_points"] > 0
    ctx.close()


# ---- the seams ----------------------------------------------------------------------------------------------------------------
def test_example_with_louvain_writes_the_restatements_ids(tmp_path):
    """examples/edge_matcher_refpoints.cpp on --make-synthetic scene 2: --louvain out.txt needs no --communities, writes the
    restatement's ids, and pipeline 1's extractor runs in front of the rest: the output differs from the run without it."""
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path, lib=cbuild.DEFAULT_LIB)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "2", d])
    s = _synth(2)[0]
    g_want, want = _simgraph_want(2, 0, s.n_seeds)
    common = [exe, os.path.join(d, "input.json"), os.path.join(d, "plgs.bin")]
    env = dict(os.environ, EG3D_LIB="")   # (the example links the default library)
    gpath, cpath = os.path.join(d, "graph.txt"), os.path.join(d, "communities.txt")
    subprocess.check_call(common + [os.path.join(d, "a.json")], env=env)
    subprocess.check_call(common + [os.path.join(d, "b.json"), "--louvain", cpath, "--match1-graph", gpath], env=env)
    assert open(gpath, "rb").read() == sref.graph_text(g_want).encode()
    assert open(cpath).read() == L.communities_text(want["ids"])
    assert open(os.path.join(d, "a.json"), "rb").read() != open(os.path.join(d, "b.json"), "rb").read()
    # without a file name nothing is written and the result is the same; --communities and --louvain exclude each other
    subprocess.check_call(common + [os.path.join(d, "c.json"), "--louvain"], env=env)
    assert open(os.path.join(d, "c.json"), "rb").read() == open(os.path.join(d, "b.json"), "rb").read()
    assert subprocess.call(common + [os.path.join(d, "e.json"), "--louvain", "--communities", cpath], env=env) != 0


def test_refapi_compute_communities(tmp_path):
    """compute_communities of include/eg3d_refapi.hpp (tests/refapi/louvain_check.cpp) on config 1: both files hold the
    restatement's text, the returned ids are the restatement's, and SimilarityGraph::communities passes its parameters on."""
    exe = cbuild.build_caller("tests/refapi/louvain_check.cpp", tmp_path, lib=cbuild.DEFAULT_LIB)
    s = _synth(1)[0]
    g_want, want = _simgraph_want(1, 0, s.n_seeds)
    assert g_want["n_nodes"] >= 10
    gpath, cpath = str(tmp_path / "graph.txt"), str(tmp_path / "communities.txt")
    out = subprocess.run([exe, "1", gpath, cpath], env=dict(os.environ, EG3D_LIB=""), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert open(gpath, "rb").read() == sref.graph_text(g_want).encode()
    assert open(cpath).read() == L.communities_text(want["ids"])
    assert [int(t) for t in out[0].split()] == want["ids"].tolist()
    one = L.louvain(g_want["n_nodes"], g_want["adj_off"], g_want["adj_node"], g_want["adj_w"], max_phases=1)
    assert [int(t) for t in out[1].split()] == one["ids"].tolist()
    assert [int(t) for t in out[2].split()] == [1, one["n_communities"]]


def test_edge_matching_detects_pipeline_1s_communities(tmp_path):
    """edge_matching() of include/eg3d_edge_matcher.hpp (tests/refapi/edge_matching_louvain_check.cpp) on synthetic config 1,
    its polylines drawn into edge images: with run_pipeline1 alone the stage stays skipped, as before; with
    pipeline1_detect_communities bit 0 of skipped_pipelines is clear, the graph file holds the text of the compatibility graph
    the same inputs give, and the communities file holds the restatement's ids on that graph."""
    import png_util
    import real_scene as rs
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path, lib=cbuild.DEFAULT_LIB)
    chk = cbuild.build_caller("tests/refapi/edge_matching_louvain_check.cpp", tmp_path, lib=cbuild.DEFAULT_LIB)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "1", d])
    _, sc, _ = _synth(1)
    edges = os.path.join(d, "edges")
    os.makedirs(edges)
    os.makedirs(os.path.join(d, "out"))
    for v in range(sc["n_views"]):
        a, b = int(sc["view_pl_off"][v]), int(sc["view_pl_off"][v + 1])
        off = sc["pl_vtx_off"][a:b + 1].astype(np.int64)
        mask = rs.rasterise(sc["vtx_xy"], off, sc["pl_valid"][a:b], sc["width"], sc["height"])
        png_util.write_png_gray(os.path.join(edges, "%04d.png" % v), mask * 255)
    gpath, cpath = os.path.join(d, "graph.txt"), os.path.join(d, "communities.txt")
    out = subprocess.run([chk, edges, os.path.join(d, "input.json"), os.path.join(d, "out") + os.sep, gpath, cpath],
                         env=dict(os.environ, EG3D_LIB=""), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert "the stage is skipped" in out.stderr.lower()
    assert [int(t) for t in lines[0].split()] == [0, 3]         # pipelines 1 and 2 skipped
    assert [int(t) for t in lines[1].split()] == [0, 2]         # bit 0 is clear
    g = {"n_nodes": int(lines[2]), "adj_off": np.array(lines[3].split(), np.uint32), "adj_node": np.array(lines[4].split(), np.uint32),
         "adj_w": np.array(lines[5].split(), np.uint32).view(np.float32)}
    assert g["n_nodes"] >= 10 and len(g["adj_node"]) == int(g["adj_off"][-1]) > 0
    assert open(gpath, "rb").read() == sref.graph_text(g).encode()
    want = L.louvain(g["n_nodes"], g["adj_off"], g["adj_node"], g["adj_w"])
    assert open(cpath).read() == L.communities_text(want["ids"])
    assert os.path.exists(os.path.join(d, "out", "out.json"))
