"""CPU: the rule "is this point of a polyline already matched?" (csrc/eg3d_matched_core.h, exported from libeg3d_host.so as
eg3d_host_is_matched) against the independent restatement tests/matched_ref.py — hand-made rows, one per rule and quirk
(M1-M4 of the header), then every sample and every epipolar hit of Synth(0)'s curve sets against the intervals the oracle's
replay leaves behind after the oracle's pipeline 3."""
import ctypes as C

import numpy as np
import pytest

import matched_ref as R
from edgegraph3d_amd import host
from oracle import binding as ob


# ---- a hand-made scene: one view, polyline 0 along the x axis with a vertex every 100 px (segments 0 .. 3), polyline 1 a
# closed one (start node == end node), polyline 2 a single vertex
def _hand_scene():
    vtx = np.asarray([[0, 0], [100, 0], [200, 0], [300, 0], [400, 0],
                      [0, 50], [100, 50], [100, 150], [0, 50],
                      [7, 7]], np.float32)
    return {"n_views": 1, "width": 1600, "height": 1200, "cam_P": np.zeros((1, 16), np.float32),
            "F": np.zeros((1, 1, 9), np.float64), "F_valid": np.zeros((1, 1), np.uint8),
            "view_pl_off": np.asarray([0, 3], np.uint32), "pl_vtx_off": np.asarray([0, 5, 9, 10], np.uint32), "vtx_xy": vtx,
            "pl_start": np.asarray([0, 2, 3], np.uint32), "pl_end": np.asarray([1, 2, 3], np.uint32),
            "pl_valid": np.ones(3, np.uint8)}


def _graph(scene, rows):
    """rows: {global polyline: [(start seg, (x, y), end seg, (x, y))]} -> the iv_* arrays of a graph dict"""
    NP = int(scene["view_pl_off"][-1])
    off, sseg, sxy, eseg, exy = [0], [], [], [], []
    for g in range(NP):
        for a, axy, b, bxy in rows.get(g, ()):
            sseg.append(a), sxy.append(axy), eseg.append(b), exy.append(bxy)
        off.append(len(sseg))
    n = len(sseg)
    return {"n_scene_polylines": NP, "iv_off": np.asarray(off, np.uint64), "iv_start_seg": np.asarray(sseg, np.uint32),
            "iv_start_xy": np.asarray(sxy, np.float32).reshape(n, 2), "iv_end_seg": np.asarray(eseg, np.uint32),
            "iv_end_xy": np.asarray(exy, np.float32).reshape(n, 2)}


A1 = (1, (110, 0), 1, (150, 0))      # start and end on segment 1
B2 = (2, (220, 0), 2, (260, 0))
Z0 = (0, (10, 0), 0, (50, 0))        # starts on segment 0
LONG = (1, (110, 0), 3, (350, 0))    # segments 1 .. 3
A12 = (1, (110, 0), 2, (250, 0))
ENDV = (1, (110, 0), 1, (200, 0))    # ends exactly on vertex 2
STARTV = (2, (200, 0), 2, (260, 0))  # starts exactly on vertex 2

# (name, row of polyline 0, (segment, x, y), expected index) — the expectation is worked out by hand from
# plg_matches_manager.cpp:54-85 and polyline_graph_2d.cpp:269-293
HAND = [
    ("M1 an interval that starts on segment 0 contains nothing (start - 1 wraps)", [Z0], (0, 30, 0), -1),
    ("M1 ... not even its own start point", [Z0], (0, 10, 0), -1),
    ("M2 strictly inside a long interval: never true", [LONG], (2, 250, 0), -1),
    ("M3 the interval that starts on the point's own segment", [A1, B2], (2, 240, 0), 1),
    ("M3 own-segment interval does not hold it, the one before ends earlier but does not reach it", [A1, B2], (2, 210, 0), -1),
    ("M3 the one before, end segment == the point's segment", [A12], (2, 230, 0), 0),
    ("M3 the one before, point past its end", [A12], (2, 270, 0), -1),
    ("M3 the one before is tested only when it ENDS on or before the point's segment", [LONG, (3, (360, 0), 3, (380, 0))],
     (2, 250, 0), -1),
    ("M4 every interval starts after the point: begin()-- in the reference, not matched here", [B2], (1, 150, 0), -1),
    ("one interval, point between start and end", [A1], (1, 130, 0), 0),
    ("one interval, point before its start on the same segment", [A1], (1, 105, 0), -1),
    ("one interval, point after its end on the same segment", [A1], (1, 160, 0), -1),
    ("one interval, point on its start", [A1], (1, 110, 0), 0),
    ("one interval, point on its end", [A1], (1, 150, 0), 0),
    ("the point is the interval's end vertex, tagged with the NEXT segment", [ENDV], (2, 200, 0), 0),
    ("... but not when the end is short of the vertex", [A1], (2, 200, 0), -1),
    ("the point is the interval's start vertex, tagged with the PREVIOUS segment: interval_contains_plp says yes, "
     "is_matched never asks (M4)", [STARTV], (1, 200, 0), -1),
    ("... nor with an interval before it (M1 empties that one)", [Z0, STARTV], (1, 200, 0), -1),
    ("empty row", [], (1, 130, 0), -1),
]


@pytest.fixture(scope="module")
def hand():
    sc = _hand_scene()
    return sc, host.SceneArrays(sc), R.Scene(sc, ob.lib())


@pytest.mark.parametrize("name,row,pt,want", HAND, ids=[h[0][:40] for h in HAND])
def test_hand_made_rows(hand, name, row, pt, want):
    sc, arr, S = hand
    seg, xy = pt[0], (np.float32(pt[1]), np.float32(pt[2]))
    v = S.vertices(0)
    ref = R.is_matched([R.Interval(*iv) for iv in row], v, seg, xy)
    got = host.is_matched(C.pointer(arr.c), _graph(sc, {0: row}), [0], [0], [seg], [xy])
    print(name, "restatement", ref, "probe", int(got[0]), "expected", want)
    assert ref == want, name
    assert int(got[0]) == want, name


def test_start_vertex_on_previous_segment_is_contained_but_not_matched(hand):
    _, _, S = hand
    assert R.interval_contains_plp(R.Interval(*STARTV), S.vertices(0), 1, (np.float32(200), np.float32(0)))
    assert R.interval_contains_plp(R.Interval(*ENDV), S.vertices(0), 2, (np.float32(200), np.float32(0)))
    assert not R.interval_contains_plp(R.Interval(*Z0), S.vertices(0), 0, (np.float32(30), np.float32(0)))  # M1


def test_closed_polyline_hits_are_answered_without_a_walk(hand):
    sc, arr, S = hand
    row = [(1, (100, 60), 1, (100, 140))]
    got = host.is_matched(C.pointer(arr.c), _graph(sc, {1: row}), [0], [1], [1], [(100, 100)])
    assert int(got[0]) == R.is_matched([R.Interval(*row[0])], S.vertices(1), 1, (np.float32(100), np.float32(100))) == 0
    assert R.jump_ok(S, 0, 1, [R.Interval(*row[0])], 0, 1, (np.float32(100), np.float32(100)))


def test_table_checks(hand):
    sc, arr, _ = hand
    p = C.pointer(arr.c)
    ok = _graph(sc, {0: [A1, B2]})
    assert list(host.is_matched(p, ok, [0], [0], [1], [(130, 0)])) == [0]
    bad = []
    g = _graph(sc, {0: [B2, A1]})                                   # start segments not ascending
    bad.append(("order", g))
    g = _graph(sc, {0: [A1, (1, (160, 0), 1, (170, 0))]})           # ... not STRICTLY ascending
    bad.append(("repeat", g))
    g = _graph(sc, {0: [(4, (400, 0), 4, (400, 0))]})               # start segment outside the polyline (segments 0 .. 3)
    bad.append(("start seg", g))
    g = _graph(sc, {0: [(1, (110, 0), 4, (400, 0))]})               # end segment outside
    bad.append(("end seg", g))
    g = _graph(sc, {2: [(0, (7, 7), 0, (7, 7))]})                   # an interval on a polyline with fewer than two vertices
    bad.append(("one vertex", g))
    g = dict(ok, iv_off=np.asarray([0, 2, 1, 2], np.uint64))        # offsets not ascending
    bad.append(("offsets", g))
    g = dict(ok, n_scene_polylines=2, iv_off=ok["iv_off"][:3])      # not the scene's number of polylines
    bad.append(("n_scene_polylines", g))
    for name, g in bad:
        with pytest.raises(ValueError):
            host.is_matched(p, g, [0], [0], [1], [(130, 0)])
            pytest.fail("accepted: " + name)
    with pytest.raises(ValueError):  # a point that is not on a segment of its polyline
        host.is_matched(p, ok, [0], [0], [4], [(400, 0)])


def test_progress_rule_refuses_an_interval_that_ends_behind_its_point(hand):
    """An interval that starts on segment 2 and ends on segment 1 passes every table check and, by the reference's rule,
    contains the point (250, 0) of segment 2; its end lies 130 px BEHIND that point, so the walk that jumps to it comes back
    to the same place for ever in the reference. Probe and restatement refuse it alike."""
    sc, arr, S = hand
    back = (2, (210, 0), 1, (120, 0))
    row = [R.Interval(*back)]
    xy = (np.float32(250), np.float32(0))
    k = R.is_matched(row, S.vertices(0), 2, xy)
    assert k == 0
    assert not R.jump_ok(S, 0, 0, row, k, 2, xy)
    with pytest.raises(R.NoProgress):
        R.walk(S, 0, 0, row)
    with pytest.raises(ValueError, match="do not belong"):
        host.is_matched(C.pointer(arr.c), _graph(sc, {0: [back]}), [0], [0], [2], [xy])
    # the same interval the right way round is fine: the walk skips it and goes on
    fwd = [R.Interval(1, (120, 0), 2, (210, 0))]
    tasks, skipped = R.walk(S, 0, 0, fwd)
    assert skipped > 0 and all(R.is_matched(fwd, S.vertices(0), s, p) < 0 for s, p in tasks)


# ---- Synth(0): the oracle's pipeline 3, the oracle's replay, every sample and hit of the 8 curve sets
@pytest.fixture(scope="module")
def synth0():
    s = host.Synth(0)
    orc = ob.Oracle(s.scene)
    cloud = orc.match(s.seeds, 0, s.n_seeds, 1)
    graph = orc.replay_matches(cloud)
    n_sets, row_off, pl_ids = s.polyline_sets()
    S = R.Scene(s.scene_np(), ob.lib())
    plain = R.stage_a(S, n_sets, row_off, pl_ids, None)  # the unskipped walk: every sample, every hit
    yield s, orc, graph, (n_sets, row_off, pl_ids), S, plain
    orc.close()
    s.close()


def _points_of(plain, V):
    """(view, pl, seg, xy) of every sample and of every epipolar hit (own-view list entries left out) of a stage A"""
    nt = plain["n_tasks"]
    smp = (plain["task_view"], plain["task_pl"], plain["task_seg"], plain["task_xy"])
    lo = plain["list_off"].astype(np.int64)
    hv = np.repeat(np.tile(np.arange(V, dtype=np.int32), nt), np.diff(lo))
    own = np.repeat(np.repeat(plain["task_view"], V), np.diff(lo)) == hv
    hit = (hv[~own], plain["hit_pl"][~own], plain["hit_seg"][~own], plain["hit_xy"][~own])
    return smp, hit


def test_probe_equals_restatement_on_synth0(synth0):
    s, orc, graph, sets, S, plain = synth0
    rows = R.rows_of(graph)
    smp, hit = _points_of(plain, S.V)
    n_matched = []
    for what, (view, pl, seg, xy) in (("samples", smp), ("hits", hit)):
        ref = np.asarray([R.is_matched(rows.get(S.gid(v, p), []), S.vertices(S.gid(v, p)), sg, (c[0], c[1]))
                          for v, p, sg, c in zip(view, pl, seg, xy)], np.int64)
        got = host.is_matched(s.scene, graph, view, pl, seg, xy)
        print("%s: %d, inside a held interval: %d (restatement), %d (probe)" % (what, len(ref), (ref >= 0).sum(), (got >= 0).sum()))
        assert np.array_equal(ref, got), what
        n_matched.append(int((ref >= 0).sum()))
    assert len(smp[0]) == 1200 and n_matched[0] == 480  # (the figures the feature was proposed with)
    assert n_matched[0] > 0 and n_matched[1] > 0


def test_restated_walk_with_an_empty_manager_is_the_oracles(synth0):
    s, orc, graph, (n_sets, row_off, pl_ids), S, plain = synth0
    V = S.V
    empty = dict(graph, iv_off=np.zeros_like(graph["iv_off"]), iv_start_seg=np.zeros(0, np.uint32),
                 iv_start_xy=np.zeros((0, 2), np.float32), iv_end_seg=np.zeros(0, np.uint32), iv_end_xy=np.zeros((0, 2), np.float32))
    assert R.same_candidates(plain, R.stage_a(S, n_sets, row_off, pl_ids, empty)) is None
    n = 0
    for r in range(n_sets * V):
        for pl in pl_ids[row_off[r]:row_off[r + 1]]:
            xy, seg = orc.polyline_samples(r % V, int(pl))
            tasks, skipped = R.walk(S, r % V, int(pl), None)
            assert skipped == 0 and [t[0] for t in tasks] == list(seg)
            assert np.array_equal(np.asarray([t[1] for t in tasks], np.float32).reshape(-1, 2).view(np.uint32), xy.view(np.uint32))
            n += len(seg)
    assert n == plain["n_tasks"] == 1200


def test_matched_stage_a_on_synth0_skips_and_filters(synth0):
    """The restatement itself: with the pipeline-3 intervals fewer samples become tasks, none of them is matched, and
    every surviving hit is unmatched."""
    s, orc, graph, (n_sets, row_off, pl_ids), S, plain = synth0
    m = R.stage_a(S, n_sets, row_off, pl_ids, graph)
    print("tasks %d -> %d, skipped %d, hits filtered %d" % (plain["n_tasks"], m["n_tasks"], m["n_samples_skipped"], m["n_hits_filtered"]))
    assert m["n_samples_skipped"] > 0 and m["n_hits_filtered"] > 0 and m["n_tasks"] < plain["n_tasks"]
    smp, hit = _points_of(m, S.V)
    for view, pl, seg, xy in (smp, hit):
        if len(view):
            assert (host.is_matched(s.scene, graph, view, pl, seg, xy) < 0).all()
