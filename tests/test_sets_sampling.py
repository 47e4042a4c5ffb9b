"""CPU: the sampling of the pipelines 1-2 extractor, pinned to something other than the oracle itself.

The extractor samples every polyline of a set every 20 px of CHORD (Euclidean distance from the previous sample, not arc
length) from its start towards its end: next_pl_point_by_distance(plp, pl.end, 20, reached_end)
(polyline_matching.cpp:153-208 with polyline_graph_2d.cpp:391-440). The oracle restates that walk in float32
(oracle_geom.hpp) and the GPU kernel k_n1_samples matches the oracle bit for bit (tests/test_gpu_polyline_sets.py). Here a
float64 numpy restatement of the same walk, written from the reference and independent of the oracle, must give the
oracle's count_set_samples per polyline and its sample positions within 1e-3 px. A sample whose walk compared a chord
within 1e-4 px of the 20 px boundary is left out (float32 and float64 may decide such a comparison differently): those
are counted, and the `exact` family puts samples on that side on purpose."""
import ctypes as C

import numpy as np

import sets_cases as cases
from edgegraph3d_amd import api, host

BOUNDARY_EPS = 1e-4


def _walk64(xy, loop):
    """(samples [(x, y, seg)], index of the first sample whose walk met the boundary or None) of a polyline walked
    towards its end. A loop (end node == start node) takes the `direction == start` branch first
    (polyline_graph_2d.cpp:398): it walks towards the start it stands on and reaches the extreme at once."""
    out, near = [], None
    if loop or len(xy) < 2:
        return out, near
    v = np.asarray(xy, np.float64)
    n = len(v)
    p, seg = v[0].copy(), 0
    while True:
        if seg >= n - 1:
            break
        touched = False
        cur = float(np.linalg.norm(v[seg + 1] - p))
        touched |= abs(cur - cases.SPLIT) < BOUNDARY_EPS
        if cur >= cases.SPLIT:
            q, qseg = p + (v[seg + 1] - p) * (cases.SPLIT / cur), seg
        else:
            i, found = seg + 1, False
            while i < n - 1:
                prev = cur
                cur = float(np.linalg.norm(v[i + 1] - p))
                touched |= abs(cur - cases.SPLIT) < BOUNDARY_EPS
                if cur >= cases.SPLIT:
                    found = True
                    break
                i += 1
            if not found:
                if touched and near is None:
                    near = len(out)  # (the extreme decision itself was on the boundary)
                break
            q, qseg = v[i] + (v[i + 1] - v[i]) * ((cases.SPLIT - prev) / (cur - prev)), i
        if touched and near is None:
            near = len(out)
        out.append((q[0], q[1], qseg))
        p, seg = q, qseg
    return out, near


def _one_polyline_sets(case):
    """one set per polyline of the scene (that polyline alone in its view's row)"""
    sets, who = [], []
    for v in range(case.V):
        for p in range(case.n_pl(v)):
            sets.append({v: [p]})
            who.append((v, p))
    return sets, who


def test_sampling_matches_a_float64_restatement_of_the_walk():
    from oracle import binding as ob
    compared = left_out = polylines = 0
    per_family = {}
    for name in ("tiny", "exact", "degenerate", "sparse"):
        case = cases.FAMILIES[name]()
        sa = case.scene_arrays()
        o = ob.Oracle(C.byref(sa.c))
        sets, who = _one_polyline_sets(case)
        n, row_off, ids = cases.to_csr(sets, case.V)
        counts = o.count_set_samples(n, row_off, ids)
        fam_left = 0
        for (v, p), cnt in zip(who, counts):
            kind = case.kind(v, p)
            xy, seg = o.polyline_samples(v, p)
            assert len(xy) == cnt, (name, v, p)
            if kind in ("invalid", "short"):
                assert cnt == 0, (name, v, p, kind)
                continue
            mine, near = _walk64(case.polyline(v, p), kind == "loop")
            polylines += 1
            if near is None:
                assert cnt == len(mine), (name, v, p, cnt, len(mine))
                upto = cnt
            else:
                upto = near
                left_out += cnt - near
                fam_left += cnt - near
            for k in range(min(upto, cnt)):
                assert abs(float(xy[k, 0]) - mine[k][0]) <= 1e-3 and abs(float(xy[k, 1]) - mine[k][1]) <= 1e-3, \
                    (name, v, p, k, xy[k], mine[k])
                assert int(seg[k]) == mine[k][2], (name, v, p, k)
            compared += min(upto, cnt)
        per_family[name] = fam_left
        # the per-set counts of the family's own sets are the sums of their polylines' counts
        n2, ro2, ids2 = case.csr()
        own = dict(zip(who, counts))
        want = [sum(int(own[(v, p)]) for v, ps in s.items() for p in ps) for s in case.sets]
        assert list(o.count_set_samples(n2, ro2, ids2)) == want, name
    assert compared >= 3000 and polylines >= 500, (compared, polylines)
    assert per_family["exact"] >= 100, per_family   # the family built for the boundary reaches it
    assert left_out < compared // 4, (left_out, compared)


def test_loops_are_not_sampled():
    """start node == end node: the walk towards `end` is the walk towards `start` (tested first in
    polyline_graph_2d.cpp:398): no sample, whatever the geometry."""
    from oracle import binding as ob
    case = cases.degenerate()
    o = ob.Oracle(C.byref(case.scene_arrays().c))
    loops = [(v, p) for v in range(case.V) for p in range(case.n_pl(v)) if case.kind(v, p) == "loop"]
    assert len(loops) >= 10
    for v, p in loops:
        assert len(case.polyline(v, p)) >= 2
        assert len(o.polyline_samples(v, p)[0]) == 0


def _product_accepts(n, row_off, ids, V):
    try:
        api.check_polyline_sets(n, row_off, ids, V)
        return True
    except api.Eg3dError:
        return False


def test_every_in_repo_producer_of_sets_emits_strictly_ascending_rows():
    """include/eg3d.h: a row is the reference's set<ulong>, strictly ascending; eg3d_match_polyline_sets refuses anything
    else. The synthetic producer (Synth.polyline_sets, also what bench.py --path sets and tools/ use) and every family of
    tests/sets_cases.py keep to it, by the Python helper and by the product's own device-free check."""
    for cfg in (0, 1, 2):
        s = host.Synth(cfg)
        n, row_off, ids = s.polyline_sets()
        assert cases.rows_strictly_ascending(n, row_off, ids, s.n_views), cfg
        assert _product_accepts(n, row_off, ids, s.n_views), cfg
    for name, fn in cases.FAMILIES.items():
        c = fn()
        n, row_off, ids = c.csr()
        assert cases.rows_strictly_ascending(n, row_off, ids, c.V), name
        assert _product_accepts(n, row_off, ids, c.V), name


def test_rows_that_are_not_sets_are_refused_without_a_device():
    """eg3d_check_polyline_sets — the part of eg3d_match_polyline_sets' argument checks that runs before any device call —
    refuses a repeated id, a swapped pair and a descending row_off with EG3D_ERR_ARG and a message, in any row (also the
    last row of the last set); sorted rows, empty rows and empty sets pass."""
    L = api.lib()
    V = 3
    ro = np.array([0, 3, 3, 4, 4, 4, 6], np.uint32)  # set 0: rows of 3, 0, 1 ids; set 1: 0, 0, 2 ids
    good = np.array([1, 4, 5, 7, 0, 9], np.uint32)
    assert _product_accepts(2, ro, good, V)
    assert _product_accepts(1, ro, good[:4], V)
    assert _product_accepts(2, np.zeros(2 * V + 1, np.uint32), np.zeros(0, np.uint32), V)
    for bad_ids, what in ((np.array([1, 4, 4, 7, 0, 9], np.uint32), b"not strictly ascending"),
                          (np.array([1, 5, 4, 7, 0, 9], np.uint32), b"not strictly ascending"),
                          (np.array([1, 4, 5, 7, 9, 9], np.uint32), b"not strictly ascending"),
                          (np.array([1, 4, 5, 7, 9, 0], np.uint32), b"not strictly ascending")):
        assert not _product_accepts(2, ro, bad_ids, V), bad_ids
        assert what in L.eg3d_last_error()
    bad_off = ro.copy()
    bad_off[2] = 1
    assert not _product_accepts(2, bad_off, good, V)
    assert b"row_off is not ascending" in L.eg3d_last_error()
    # ids of different rows need no order between them (row 3 starts lower than row 0 ends)
    assert _product_accepts(2, ro, np.array([1, 4, 5, 0, 2, 3], np.uint32), V)


def test_unit_cut_restatement_on_the_bound_families():
    """A consistency check of the TEST DATA, not of the product: the ranges of the bound families are cut, by the
    restatement sets_cases.units_expected, into the number of units each declares (exactly max_items ids in one unit, one
    more in two, a set above the bound alone). The product's cut is checked on the device, through
    eg3d_last_device_output().complete (tests/test_gpu_polyline_sets.py)."""
    for name in ("bound_lo", "bound_hi"):
        c = cases.FAMILIES[name]()
        n, row_off, ids = c.csr()
        mx = c.meta["max_items"]
        assert (c.V < 64) == (mx == cases.MAX_ITEMS_LO)
        for b, e, units in c.units:
            assert cases.units_expected(row_off, c.V, b, e, mx) == units, (name, b, e)
