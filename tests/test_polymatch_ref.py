"""CPU tests of the polyline matcher (eg3d_match_polylines_closeness): the Python restatement (tests/polymatch_ref.py) is pinned
against the oracle's grids before its 10 px map is trusted; the rule per reference point and the order of the components are
checked on hand-made inputs (tests/polymatch_cases.py); the parts of the C ABI that need no device run here."""
import ctypes as C
import os

import numpy as np
import pytest

import polymatch_cases as pc
import polymatch_ref as ref
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, build, host
from oracle import binding as ob


# ---- the map restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,cell", [(0, 30.0), (1, 4.0)])
def test_map_restatement_equals_oracle_on_config0(which, cell):
    s = host.Synth(0)
    sc = s.scene_np()
    orc = ob.Oracle(s.scene)
    for v in range(sc["n_views"]):
        ncols, nrows, off, ids = orc.grid(v, which)
        g = ref.build_map(sc, v, cell)
        assert (g[0], g[1]) == (ncols, nrows)
        assert np.array_equal(g[2], off) and np.array_equal(g[3], ids), v


@pytest.mark.parametrize("which,cell", [(0, 30.0), (1, 4.0)])
def test_map_restatement_equals_oracle_on_a_real_view(which, cell):
    """One dtu006 edge image -> polylines by the oracle's builder -> both maps."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dtu006_edges", "0000.png")
    mask = host.png_edge_mask(path)
    v = ob.plg_from_mask(mask)
    NP = len(v["pl_start"])
    sc = {"n_views": 1, "width": mask.shape[1], "height": mask.shape[0], "cam_P": np.eye(4, dtype=np.float32).reshape(1, 16),
          "F": np.zeros((1, 1, 9)), "F_valid": np.zeros((1, 1), np.uint8), "view_pl_off": np.array([0, NP], np.uint32),
          "pl_vtx_off": v["pl_vtx_off"], "vtx_xy": v["vtx_xy"], "pl_start": v["pl_start"], "pl_end": v["pl_end"],
          "pl_valid": v["pl_valid"]}
    sa = host.SceneArrays(sc)
    ncols, nrows, off, ids = ob.Oracle(C.pointer(sa.c)).grid(0, which)
    g = ref.build_map(sc, 0, cell)
    assert (g[0], g[1]) == (ncols, nrows)
    assert np.array_equal(g[2], off) and np.array_equal(g[3], ids)


# ---- the rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,views,results,accepted", pc.RULE_TABLE, ids=[r[0] for r in pc.RULE_TABLE])
def test_rule_table(name, views, results, accepted):
    assert (ref.refpoint_rule(views, results) is not None) == accepted


def test_rule_counts_distinct_pairs_and_orders_them():
    assert ref.refpoint_rule([2, 0, 0, 1], [[(5, 2.0)], [(7, 2.0)], [(7, 2.0)], [(1, 2.0)]]) == [(0, 7), (1, 1), (2, 5)]


# ---- component order --------------------------------------------------------------------------------------------------
def _by_key(accepted, n_views, view_pl_off):
    """The order-independent statement the device uses: a component's key is the minimum over its nodes of (first accepting
    point, global polyline index); components ascend by key, their polylines by (view, id)."""
    first, parent = {}, {}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for pid, pairs in reversed(accepted):      # (any order: reversed on purpose)
        for (v, pl) in pairs:
            g = view_pl_off[v] + pl
            first[g] = min(first.get(g, pid), pid)
            parent.setdefault(g, g)
        g0 = view_pl_off[pairs[0][0]] + pairs[0][1]
        for (v, pl) in pairs[1:]:
            a, b = find(g0), find(view_pl_off[v] + pl)
            if a != b:
                parent[max(a, b)] = min(a, b)
    comps = {}
    for g in first:
        comps.setdefault(find(g), []).append(g)
    order = sorted(comps.values(), key=lambda c: min((first[g], g) for g in c))
    row_off, pl_ids = [0], []
    for c in order:
        for v in range(n_views):
            pl_ids.extend(sorted(g - view_pl_off[v] for g in c if view_pl_off[v] <= g < view_pl_off[v + 1]))
            row_off.append(len(pl_ids))
    return len(order), row_off, pl_ids


def _by_stack_walk(accepted, n_views):
    nodes, adj = ref.match_graph(accepted)
    comps = ref.components_stack_walk(len(nodes), adj)
    row_off, pl_ids = ref.sets_from_components(nodes, comps, n_views)
    return len(comps), list(row_off), list(pl_ids)


@pytest.mark.parametrize("name", list(pc.COMPONENT_CASES))
def test_component_order_cases(name):
    accepted = pc.COMPONENT_CASES[name]
    vpo = [0, 10, 20, 30, 40]
    assert _by_key(accepted, 4, vpo) == _by_stack_walk(accepted, 4)


def test_component_order_hand_checked():
    """Interleaved creation: point 0 opens {(0,5),(1,5)}, point 1 opens {(0,1),(1,1)}; the first component is the one point 0
    opened although its polyline ids are larger."""
    n, row_off, pl_ids = _by_stack_walk(pc.COMPONENT_CASES["two components created in interleaved order"], 4)
    assert n == 2
    assert pl_ids == [5, 5, 5, 1, 1, 0] and row_off == [0, 1, 2, 3, 3, 4, 5, 6, 6]
    n, row_off, pl_ids = _by_stack_walk(pc.COMPONENT_CASES["a later point merges two earlier components"], 4)
    assert n == 2 and pl_ids == [2, 9, 2, 9, 4, 4]


def test_component_order_random_graphs():
    rng = np.random.default_rng(20240917)
    for _ in range(200):
        accepted = pc.random_component_case(rng)
        assert _by_key(accepted, 4, [0, 6, 12, 18, 24]) == _by_stack_walk(accepted, 4), accepted


# ---- the C ABI, without a device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("libname", ["HIP_LIB", "HIP_LIB_DLT4X4"])
def test_abi_symbols_in_both_libraries(libname):
    path = getattr(build, libname)
    if not os.path.exists(path):
        (build.build_hip if libname == "HIP_LIB" else build.build_hip_dlt4x4)()
    L = C.CDLL(path)
    for name in ("eg3d_match_polylines_closeness", "eg3d_free_polyline_matches"):
        assert hasattr(L, name), name
        assert name in api.EXPORTED_SYMBOLS
    needed = os.popen("readelf -d %s" % path).read()
    assert "libeg3d_host" not in needed


def test_abi_small_struct_size_is_refused_before_anything_else():
    L = api.lib()
    st = D.PolymatchStats()
    st.struct_size = C.sizeof(D.PolymatchStats) - 4
    m = D.PolylineMatches()
    assert L.eg3d_match_polylines_closeness(None, None, 0, 0, C.byref(m), C.byref(st)) == -1
    assert b"struct_size" in L.eg3d_last_error()
    assert st.struct_size == C.sizeof(D.PolymatchStats) - 4 and not m.row_off
    st.struct_size = C.sizeof(D.PolymatchStats)
    assert L.eg3d_match_polylines_closeness(None, None, 0, 0, C.byref(m), C.byref(st)) == -1   # (no context)
    L.eg3d_free_polyline_matches(C.byref(m))   # (an empty result may be freed)
    L.eg3d_free_polyline_matches(None)


def test_restatement_result_passes_check_polyline_sets():
    """The restatement's sets on the hand-built rule scene are a valid eg3d_polyline_sets (the device result must equal them:
    tests/test_gpu_polymatch.py)."""
    sc, seeds = pc.rule_scene()
    r = ref.Matcher(sc).match(seeds, 0, len(seeds[0]) - 1)
    assert r["n_sets"] >= 1 and len(r["refpoints"]) >= 3
    api.check_polyline_sets(r["n_sets"], r["row_off"], r["pl_ids"], sc["n_views"])


def test_rule_scene_covers_the_rule_and_a_merge():
    """Bookkeeping of the hand-built device scene (tests/test_gpu_polymatch.py): the polyline count, the share, min < max / 3
    and fewer than two pairs each reject one of its points, and a later point merges two earlier components. (A rejection by
    max > 3 min alone needs distances one ulp apart: the rule table holds it, and the device test feeds it to the kernel.)"""
    sc, seeds = pc.rule_scene()
    m = ref.Matcher(sc)
    n = len(seeds[0]) - 1
    reasons = {ref.reject_reason(p[1], p[2]) for p in m.entry_results(seeds, 0, n)}
    assert {"maxpl", "share", "min", "two", None} <= reasons
    want = m.match(seeds, 0, n)
    assert want["n_sets"] == 2 and len(want["refpoints"]) == 8


def test_rule_table_holds_a_row_only_the_max_test_rejects():
    rows = [r for r in pc.RULE_TABLE if ref.reject_reason(r[1], r[2]) == "max"]
    assert len(rows) >= 1 and not any(r[3] for r in rows)
