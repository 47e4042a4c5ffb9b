"""-m gpu: eg3d_similarity_graph against the Python restatement of the reference (tests/simgraph_ref.py; its searches are
tests/polymatch_ref.py's, pinned against the oracle by tests/test_polymatch_ref.py). Every array of eg3d_simgraph is compared
for exact equality, the weights by their bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cbuild
import polymatch_cases as pc
import polymatch_ref as pref
import simgraph_cases as sc
import simgraph_ref as ref
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host
from oracle import binding as ob
from parity_util import compare_edgepoints

pytestmark = pytest.mark.gpu

ARRAYS = ("node_view", "node_pl", "adj_off", "adj_node", "adj_w", "point_weight", "cp_off", "cp_view", "cp_pl", "cr_off", "cr_point")
_REF = {}   # per scene: (matcher, the per-entry search results of all its seeds), computed once and never modified


def _entries(name, scene, seeds):
    if name not in _REF:
        m = pref.Matcher(scene)
        _REF[name] = (m, m.entry_results(seeds, 0, len(seeds[0]) - 1))
    return _REF[name]


def _want(name, scene, seeds, b, e):
    g = ref.similarity_graph(scene, _entries(name, scene, seeds)[1][b:e])
    g["seed_begin"] = b
    return g


def _same(got, want):
    for k in ("n_nodes", "n_points", "n_polylines", "seed_begin"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    st = got["stats"]
    assert st["n_nodes"] == want["n_nodes"] and 2 * st["n_edges"] == len(want["adj_node"])
    assert st["n_pair_instances"] == want["n_pair_instances"]


def _context(scene_ptr, budget=None):
    """A fresh context; EG3D_SIMGRAPH_PAIR_BUDGET is read when a context is created."""
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    old = os.environ.pop("EG3D_SIMGRAPH_PAIR_BUDGET", None)
    try:
        if budget is not None:
            os.environ["EG3D_SIMGRAPH_PAIR_BUDGET"] = str(budget)
        return api.Context(scene_ptr)
    finally:
        os.environ.pop("EG3D_SIMGRAPH_PAIR_BUDGET", None)
        if old is not None:
            os.environ["EG3D_SIMGRAPH_PAIR_BUDGET"] = old


def _small_budget(n_inst):
    return max(1, n_inst // 3)


HAND = [(pc, "rule_scene"), (pc, "crowded_scene"), (pc, "boundary_sample_scene"), (sc, "weights_scene"), (sc, "order_scene"),
        (sc, "long_polyline_scene")]


@pytest.mark.parametrize("mod,name", HAND, ids=[h[1] for h in HAND])
def test_hand_built_scenes(mod, name):
    """The polyline matcher's hand scenes (more than 64 polylines in one window, so the list crosses a merge batch;
    observations on cell boundaries and outside the image; an invalid polyline; a doubled view) and this feature's (a point
    without a close polyline, an edge inside a view, w < 1, the order-sensitive sums, a close_refpoints row of 80 and edge
    lists of 75 and 70). Whole range with the default budget and with one that cuts the pair instances into 3 chunks or more
    (boundary_sample_scene has a single pair instance: one chunk), a sub-range, and every point alone."""
    scene, seeds = getattr(mod, name)()
    sa, sd = host.SceneArrays(scene), host.SeedsArrays(*seeds)
    n = len(seeds[0]) - 1
    want = _want(name, scene, seeds, 0, n)
    ctx = _context(C.pointer(sa.c))
    got = ctx.similarity_graph(C.pointer(sd.c))
    _same(got, want)
    assert got["stats"]["n_entries"] == len(seeds[1])
    assert got["stats"]["n_chunks"] == (1 if want["n_pair_instances"] else 0)
    for (b, e) in [(n // 3, n - n // 4)] + [(r, r + 1) for r in range(n)]:
        _same(ctx.similarity_graph(None, b, e), _want(name, scene, seeds, b, e))
    ctx.close()
    n_inst = want["n_pair_instances"]
    budget = _small_budget(n_inst)
    ctx = _context(C.pointer(sa.c), budget)
    chunked = ctx.similarity_graph(C.pointer(sd.c))
    _same(chunked, want)
    assert chunked["stats"]["n_chunks"] == -(-n_inst // budget)
    assert chunked["stats"]["n_chunks"] >= 3 or n_inst < 3
    if name != "boundary_sample_scene":
        assert chunked["stats"]["n_chunks"] >= 3
    b, e = n // 3, n - n // 4
    _same(ctx.similarity_graph(None, b, e), _want(name, scene, seeds, b, e))
    ctx.close()


def test_long_polyline_scene_crosses_a_wavefront():
    """What the long scene is for, checked on the restatement: a close_refpoints row longer than 64 and, for the edge
    (0,0)-(1,0), lists A and B longer than 64 and of unequal length."""
    scene, seeds = sc.long_polyline_scene()
    g = _want("long_polyline_scene", scene, seeds, 0, len(seeds[0]) - 1)
    row = g["cr_point"][int(g["cr_off"][0]):int(g["cr_off"][1])].tolist()
    assert len(row) == 80
    off, view = seeds[0], seeds[1]
    lists = lambda r, v: v in view[int(off[r]):int(off[r + 1])].tolist()
    g10 = int(scene["view_pl_off"][1])
    A = [r for r in row if lists(r, 1)]
    B = [r for r in g["cr_point"][int(g["cr_off"][g10]):int(g["cr_off"][g10 + 1])].tolist() if lists(r, 0)]
    assert (len(A), len(B)) == (75, 70)


class Synth:
    def __init__(self, cfg):
        self.s = host.Synth(cfg)
        self.scene = self.s.scene_np()
        self.seeds = self.s.seeds_np()
        self.name = "config%d" % cfg


C2_SEEDS = 2000    # all of C2: the restatement takes about 3 s on the CPU for them


def test_c2():
    """Synthetic config 2 (the C2-shaped scene), its first C2_SEEDS seeds, with the default budget and in chunks."""
    y = Synth(2)
    assert y.s.n_seeds >= C2_SEEDS
    want = _want(y.name, y.scene, y.seeds, 0, C2_SEEDS)
    assert want["n_nodes"] > 500 and want["n_pair_instances"] > 5000
    ctx = _context(y.s.scene)
    ctx.upload_seeds(y.s.seeds)
    _same(ctx.similarity_graph(None, 0, C2_SEEDS), want)
    _same(ctx.similarity_graph(None, 700, 1300), _want(y.name, y.scene, y.seeds, 700, 1300))
    ctx.close()
    ctx = _context(y.s.scene, _small_budget(want["n_pair_instances"]))
    ctx.upload_seeds(y.s.seeds)
    chunked = ctx.similarity_graph(None, 0, C2_SEEDS)
    _same(chunked, want)
    assert chunked["stats"]["n_chunks"] >= 3
    ctx.close()


def test_refusals():
    """A view id outside the rig: EG3D_ERR_ARG, the outputs untouched, and the next valid call is correct. An empty range
    and a range without a close polyline: an empty graph."""
    y = Synth(0)
    n = y.s.n_seeds
    ctx = _context(y.s.scene)
    want = _want(y.name, y.scene, y.seeds, 0, n)
    _same(ctx.similarity_graph(y.s.seeds), want)
    off, view, xy = [a.copy() for a in y.seeds]
    view[5] = y.scene["n_views"]
    bad = host.SeedsArrays(off, view, xy)
    g, st = D.Simgraph(), D.SimgraphStats()
    st.struct_size = C.sizeof(D.SimgraphStats)
    st.n_entries = 12345
    rc = api.lib().eg3d_similarity_graph(ctx._h, C.pointer(bad.c), 0, n, C.byref(g), C.byref(st))
    assert rc == -1 and b"view id" in api.lib().eg3d_last_error()
    assert not g.adj_off and not g.node_view and not g.cr_off and g.n_nodes == 0 and g.n_points == 0 and st.n_entries == 12345
    _same(ctx.similarity_graph(None, 0, n), want)          # the refused seeds did not replace the uploaded ones
    _same(ctx.similarity_graph(y.s.seeds), want)
    empty = ctx.similarity_graph(None, 7, 7)
    assert empty["n_nodes"] == 0 and empty["adj_off"].tolist() == [0] and empty["n_points"] == 0
    assert empty["cp_off"].tolist() == [0] and len(empty["cr_off"]) == empty["n_polylines"] + 1 and not empty["cr_off"].any()
    ctx.close()
    scene, seeds = sc.weights_scene()
    sa, sd = host.SceneArrays(scene), host.SeedsArrays(*seeds)
    ctx = _context(C.pointer(sa.c))
    none = ctx.similarity_graph(C.pointer(sd.c), 1, 2)     # point 1 has no close polyline
    _same(none, _want("weights_scene", scene, seeds, 1, 2))
    assert none["n_nodes"] == 0 and none["adj_off"].tolist() == [0] and none["point_weight"].tolist() == [0.0]
    ctx.close()


@pytest.mark.parametrize("first", ["graph", "closeness"])
def test_both_matchers_share_the_map(first):
    """Both matchers on one context and on a clone, in either order: the 10 px map is built by the first call only, and a
    compatibility-graph call between two closeness calls does not change their result."""
    y = Synth(0)
    n = y.s.n_seeds
    want = _want(y.name, y.scene, y.seeds, 0, n)
    k9_want = _entries(y.name, y.scene, y.seeds)[0].match(y.seeds, 0, n)
    ctx = _context(y.s.scene)
    ctx.upload_seeds(y.s.seeds)

    def k9(c):
        got = c.match_polylines_closeness(None, 0, n)
        for k in ("refpoints", "row_off", "pl_ids"):
            assert np.array_equal(got[k], k9_want[k]), k
        return got["stats"]["ms_grid"]

    def k10(c):
        got = c.similarity_graph(None, 0, n)
        _same(got, want)
        return got["stats"]["ms_grid"]

    calls = [k10, k9] if first == "graph" else [k9, k10]
    assert calls[0](ctx) > 0.0
    assert calls[1](ctx) == 0.0
    clone = ctx.clone()
    for c in (clone, ctx):
        assert k9(c) == 0.0 and k10(c) == 0.0 and k9(c) == 0.0
    clone.close()
    ctx.close()


def test_end_to_end_through_the_file_seam(tmp_path):
    """Config 0: the graph is written as the reference writes it (the text equals the restatement's); the restatement's
    connected components stand in for the communities and go through the communities file; the sets built from them go
    into eg3d_match_polyline_sets, and the cloud equals the oracle's extractor on the restatement's sets."""
    y = Synth(0)
    n = y.s.n_seeds
    V = y.scene["n_views"]
    want = _want(y.name, y.scene, y.seeds, 0, n)
    ctx = _context(y.s.scene)
    got = ctx.similarity_graph(y.s.seeds)
    _same(got, want)
    gpath, cpath = str(tmp_path / "graph.txt"), str(tmp_path / "communities.txt")
    host.write_compat_graph(gpath, got)
    assert open(gpath, "rb").read() == ref.graph_text(want).encode()
    ids = ref.component_ids(want)
    assert ids.max() >= 1          # (config 0's graph has two components)
    open(cpath, "w").write("".join("%d\n" % i for i in ids))
    n_sets, row_off, pl_ids = host.sets_from_communities(got, host.read_communities(cpath), V)
    w_sets, w_off, w_ids = ref.sets_from_communities(want, ids, V)
    assert n_sets == w_sets and np.array_equal(row_off, w_off) and np.array_equal(pl_ids, w_ids)
    api.check_polyline_sets(n_sets, row_off, pl_ids, V)
    cloud = ctx.match_polyline_sets(n_sets, row_off, pl_ids)
    orc = ob.Oracle(y.s.scene).match_polyline_sets(w_sets, w_off, w_ids)
    rep = compare_edgepoints(orc, cloud)
    assert rep["ok"], rep["msgs"]
    assert cloud["n_points"] > 0
    ctx.close()


def test_example_writes_the_restatements_graph_file(tmp_path):
    """examples/edge_matcher_refpoints.cpp on --make-synthetic scene 2: --match1-graph writes the restatement's text; with
    --communities (the restatement's components) pipeline 1's extractor runs in front of the rest, and the output differs
    from the run without it."""
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path, lib=cbuild.DEFAULT_LIB)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "2", d])
    y = Synth(2)
    want = _want(y.name, y.scene, y.seeds, 0, y.s.n_seeds)
    common = [exe, os.path.join(d, "input.json"), os.path.join(d, "plgs.bin")]
    env = dict(os.environ, EG3D_LIB="")   # (the example links the default library)
    gpath, cpath = os.path.join(d, "graph.txt"), os.path.join(d, "communities.txt")
    subprocess.check_call(common + [os.path.join(d, "a.json"), "--match1-graph", gpath], env=env)
    assert open(gpath, "rb").read() == ref.graph_text(want).encode()
    open(cpath, "w").write("".join("%d\n" % i for i in ref.component_ids(want)))
    subprocess.check_call(common + [os.path.join(d, "b.json"), "--match1-graph", gpath, "--communities", cpath], env=env)
    assert open(gpath, "rb").read() == ref.graph_text(want).encode()
    assert open(os.path.join(d, "a.json"), "rb").read() != open(os.path.join(d, "b.json"), "rb").read()
    assert subprocess.call(common + [os.path.join(d, "e.json"), "--communities", os.path.join(d, "missing.txt")], env=env) != 0


def test_refapi_functions_equal_the_restatement(tmp_path):
    """The pipeline 1 functions of include/eg3d_refapi.hpp (tests/refapi/simgraph_check.cpp) on config 1: the graph file,
    close_polylines, close_refpoints and the sets from community ids are the restatement's."""
    exe = cbuild.build_caller("tests/refapi/simgraph_check.cpp", tmp_path, lib=cbuild.DEFAULT_LIB)
    y = Synth(1)
    V = y.scene["n_views"]
    want = _want(y.name, y.scene, y.seeds, 0, y.s.n_seeds)
    assert want["n_nodes"] >= 10
    ids = ref.component_ids(want)
    ids[0] = -1                                   # a dropped node
    gpath, cpath = str(tmp_path / "graph.txt"), str(tmp_path / "communities.txt")
    open(cpath, "w").write("".join("%d\n" % i for i in ids))
    out = subprocess.run([exe, "1", gpath, cpath], env=dict(os.environ, EG3D_LIB=""), capture_output=True, text=True,
                         check=True).stdout
    assert open(gpath, "rb").read() == ref.graph_text(want).encode()
    lines = out.split("\n")
    n, npl = want["n_points"], want["n_polylines"]
    for i in range(n):
        a, b = int(want["cp_off"][i]), int(want["cp_off"][i + 1])
        assert lines[i].split() == ["%d:%d" % (v, p) for v, p in zip(want["cp_view"][a:b], want["cp_pl"][a:b])], i
    for g in range(npl):
        a, b = int(want["cr_off"][g]), int(want["cr_off"][g + 1])
        assert [int(t) for t in lines[n + g].split()] == want["cr_point"][a:b].tolist(), g
    assert lines[n + npl] == "sets"
    n_sets, row_off, pl_ids = ref.sets_from_communities(want, ids, V)
    rows = [[int(t) for t in l.split()] for l in lines[n + npl + 1:n + npl + 1 + n_sets * V]]
    assert len(lines) == n + npl + 2 + n_sets * V
    for k, row in enumerate(rows):
        assert row == pl_ids[row_off[k]:row_off[k + 1]].tolist(), k
