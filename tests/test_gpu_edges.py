"""-m gpu: K17, eg3d_edge_chains_device / eg3d_edge_chains (include/eg3d/edges.h), byte for byte against the sequential
statement eg3d_host_edge_chains, stats counts included, once per product library:
  * every graph of tests/edges_cases.py and 10 of the random ones, simplified and unsimplified — either side of the wavefront
    (63 / 64 / 65), of the LDS staging limit (1025 polylines) and of every rule of the trace;
  * the refusals, an earlier result of the context intact afterwards;
  * on C2: match_refpoints(device_only) -> replay_device(to_host=False) -> edge_chains_device() equals the host statement on
    the fetched graph; the same on the graph eg3d_replay_accumulate leaves;
  * the cloud, the replay graph and a following match_polyline_sets(matched=g) are the same bytes with and without the call."""
import ctypes as C

import numpy as np
import pytest

import edges_cases as ec
import edges_ref as er
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host

pytestmark = pytest.mark.gpu

CASES = ec.cases()
RANDOM = dict(list(ec.random_cases().items())[:10])
_WANT = {}     # (name, simplify) -> the host statement's result, computed once
_CTX = {}      # form -> api.Context on host.Synth(0)
_C2 = {}       # form -> (synth, context)
_KEEP = []
CLOUD_ARRAYS = ("X", "obs_off", "obs_view", "obs_pl", "obs_seg", "obs_xy", "key")
GRAPH_ARRAYS = tuple(k for k, _ in D.GRAPH3D_ARRAYS)


def _ctx(form):
    if form not in _CTX:
        assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
        s = host.Synth(0)
        _KEEP.append(s)
        _CTX[form] = api.Context(s.scene)
    return _CTX[form]


def _c2(form):
    if form not in _C2:
        assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
        s = host.Synth(2)
        _C2[form] = (s, api.Context(s.scene))
    return _C2[form]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    import forms
    for rows in set(_CTX) | set(_C2):
        with forms.product_form(rows):   # eg3d_destroy of the library that created the context
            if rows in _CTX:
                _CTX[rows].close()
            if rows in _C2:
                _C2[rows][1].close()
    _CTX.clear()
    _C2.clear()
    _KEEP.clear()


def _want(name, g, max_dist, on):
    if (name, on) not in _WANT:
        _WANT[(name, on)] = host.edge_chains(g, max_dist, simplify=on)
    return _WANT[(name, on)]


def _fetch(dv):
    """The arrays a DeviceEdgeChains views, copied back by the test."""
    def get(ptr, n, dtype):
        a = np.empty(int(n), dtype)
        if a.nbytes:
            assert api._hip().hipMemcpy(a.ctypes.data, C.c_void_p(ptr), a.nbytes, 2) == 0
        return a
    n = int(dv.n_chains)
    return {"chain_off": get(dv.chain_off, n + 1, np.uint64), "chain_node": get(dv.chain_node, dv.n_vertices, np.uint32),
            "flags": get(dv.chain_flags, n, np.uint32), "s_off": get(dv.s_off, n + 1, np.uint64),
            "s_node": get(dv.s_node, dv.n_kept, np.uint32), "length": get(dv.length, n, np.float32)}


@pytest.mark.parametrize("on", (True, False), ids=("simplified", "traced"))
@pytest.mark.parametrize("name", sorted(CASES) + sorted(RANDOM))
def test_graph_against_the_host_statement(eg3d_form, name, on):
    g, max_dist = CASES[name] if name in CASES else RANDOM[name]
    want = _want(name, g, max_dist, on)
    got = _ctx(eg3d_form).edge_chains(g, max_dist, simplify=on)
    assert er.difference(got, want) is None, (name, on, er.difference(got, want))
    assert got["stats"]["struct_size"] == C.sizeof(D.EdgesStats)
    back = _fetch(got["device"])                     # the device view holds what the host copy holds
    back["stats"] = got["stats"]
    assert er.difference(back, want) is None, (name, on, "device view", er.difference(back, want))


def test_refusals_leave_an_earlier_result_intact(eg3d_form):
    ctx = _ctx(eg3d_form)
    g, max_dist = CASES["star_1_2_5"]
    first = ctx.edge_chains(g, max_dist)
    want = _want("star_1_2_5", g, max_dist, True)
    L = api.lib()

    def refused(graph, d):
        ga = D.EdgesGraphArrays(graph)
        ch, dv, st = D.EdgeChains(), D.DeviceEdgeChains(), D.EdgesStats()
        C.memset(C.byref(ch), 0xA5, C.sizeof(ch))
        C.memset(C.byref(dv), 0x5A, C.sizeof(dv))
        st.struct_size, st.n_chains = C.sizeof(D.EdgesStats), 0x1234
        before = bytes(ch), bytes(dv)
        rc = L.eg3d_edge_chains(ctx._h, C.byref(ga.c), C.c_float(d), 1, C.byref(dv), C.byref(ch), C.byref(st))
        assert rc == -1, rc
        assert (bytes(ch), bytes(dv)) == before and st.n_chains == 0x1234
        back = _fetch(first["device"])
        back["stats"] = first["stats"]
        assert er.difference(back, want) is None, er.difference(back, want)

    for name, bad in sorted(ec.broken_graphs().items()):
        refused(bad, 0.01)
    for d in (float("nan"), -0.01, float("inf")):
        refused(g, d)
    # no graph given and no replay on this context yet: refused as well (this context never replayed)
    fresh = api.Context(_KEEP[0].scene)
    try:
        with pytest.raises(api.Eg3dError, match="rc=-1"):
            fresh.edge_chains_device()
    finally:
        fresh.close()
    again = ctx.edge_chains(g, max_dist)             # ... and the context works on
    assert er.difference(again, want) is None


def _same_arrays(a, b, keys, what):
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def test_c2_resident_graph_and_what_the_call_leaves_alone(eg3d_form):
    s, ctx = _c2(eg3d_form)
    sets = s.polyline_sets()
    end = min(int(sets[0]), 4)
    # what a following extractor call gives WITHOUT an edge-chains call in between
    ctx.match_refpoints(s.seeds, device_only=True)
    _, dv, _ = ctx.replay_device(to_host=False)
    plain = ctx.match_polyline_sets(*sets, 0, end, matched=dv)
    # the same with the call
    r = ctx.match_refpoints(s.seeds, device_only=True)
    _, dv, rst = ctx.replay_device(to_host=False)
    cloud0, graph0 = ctx.fetch_device_output(), ctx.fetch_device_graph(dv)
    for max_dist, on in ((0.01, True), (0.05, True), (0.01, False)):
        got = ctx.edge_chains_device(max_dist=max_dist, simplify=on)         # graph=None: the last replay's
        want = host.edge_chains(graph0, max_dist, simplify=on)
        assert er.difference(got, want) is None, (max_dist, on, er.difference(got, want))
        given = ctx.edge_chains_device(dv, max_dist=max_dist, simplify=on)
        assert er.difference(given, want) is None
    st = got["stats"]
    print("C2: %d points -> %d nodes, %d polylines -> %d chains (%d rings, %d loops), longest %d; trace %.3f ms, simplify %.3f ms, "
          "copy %.3f ms" % (r["n_points"], rst["n_nodes"], rst["n_polylines"], st["n_chains"], st["n_rings"], st["n_loops_dropped"],
                            st["longest_chain"], st["ms_trace"], st["ms_simplify"], st["ms_copy"]))
    assert st["n_chains"] > 0 and st["longest_chain"] > 2
    only_dev = ctx.edge_chains_device(to_host=False)
    assert "chain_off" not in only_dev and only_dev["stats"]["n_chains"] == host.edge_chains(graph0, 0.01)["stats"]["n_chains"]
    _same_arrays(ctx.fetch_device_output(), cloud0, CLOUD_ARRAYS, "cloud")
    _same_arrays(ctx.fetch_device_graph(dv), graph0, GRAPH_ARRAYS, "replay graph")
    after = ctx.match_polyline_sets(*sets, 0, end, matched=dv)
    _same_arrays(after, plain, CLOUD_ARRAYS, "match_polyline_sets(matched=g)")
    assert after["n_points"] == plain["n_points"]


def test_c2_accumulated_graph(eg3d_form):
    s, ctx = _c2(eg3d_form)
    n = s.n_seeds
    dva = None
    for i, (b, e) in enumerate(((0, n // 2), (n // 2, n))):
        ctx.match_refpoints(s.seeds, b, e, device_only=True)
        _, dva, _ = ctx.replay_accumulate(None, reset=(i == 0), to_host=False)
    graph = ctx.fetch_device_graph(dva)
    for on in (True, False):
        got = ctx.edge_chains_device(dva, max_dist=0.02, simplify=on)
        want = host.edge_chains(graph, 0.02, simplify=on)
        assert er.difference(got, want) is None, (on, er.difference(got, want))
    assert got["stats"]["n_chains"] > 0
    _same_arrays(ctx.fetch_device_graph(dva), graph, GRAPH_ARRAYS, "accumulated graph")
