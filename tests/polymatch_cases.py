"""Hand-made inputs of the polyline-matcher tests (tests/test_polymatch_ref.py on the CPU, tests/test_gpu_polymatch.py on the
device). Data only: the expected results come from tests/polymatch_ref.py."""
import numpy as np

F32 = np.float32


def _ulp(x, n):
    return F32(np.nextafter(F32(x), F32(np.inf if n > 0 else -np.inf)))


# ---- the rule on hand-made per-entry results: (name, track view ids, per entry [(polyline, distance)], accepted?) ----------
def _e(pl, d):
    return [(pl, F32(d))]


RULE_TABLE = [
    ("maxpl 0: no entry finds a polyline", [0, 1, 2], [[], [], []], False),
    ("maxpl 1: all entries find one", [0, 1, 2], [_e(3, 2), _e(4, 2), _e(5, 3)], True),
    ("maxpl 2: one entry finds two", [0, 1, 2], [_e(3, 2), [(4, F32(2)), (7, F32(3))], _e(5, 3)], False),
    ("n 3: 2 of 3 is below 2.1", [0, 1, 2], [_e(3, 2), _e(4, 2), []], False),
    ("n 3: 3 of 3", [0, 1, 2], [_e(3, 2), _e(4, 2), _e(1, 2)], True),
    # (`size() < n * 0.7` with n = 4 compares 3 with 2.8: the reference does not reject here)
    ("n 4: 3 of 4 is above 2.8", [0, 1, 2, 3], [_e(3, 2), _e(4, 2), _e(1, 2), []], True),
    ("n 4: 2 of 4", [0, 1, 2, 3], [_e(3, 2), _e(4, 2), [], []], False),
    # (10 * 0.7 in double: 0.7 is 7 - 2^-51 tenths below, the product lies halfway between 7 - 2^-50 and 7 and rounds to the
    # even 7.0, so 7 < 7.0 is false)
    ("n 10: 7 of 10 is not below 10 * 0.7 == 7.0", list(range(10)), [_e(1, 2)] * 7 + [[]] * 3, True),
    ("n 10: 6 of 10", list(range(10)), [_e(1, 2)] * 6 + [[]] * 4, False),
    ("n 10: 8 of 10", list(range(10)), [_e(1, 2)] * 8 + [[]] * 2, True),
    ("|S| = 1 on a track of one", [0], [_e(3, 2)], False),
    ("ratio exactly 3", [0, 1], [_e(3, 1), _e(4, 3)], True),
    ("max one ulp above 3 min", [0, 1], [_e(3, 1), _e(4, _ulp(3, +1))], False),
    ("max one ulp below 3 min", [0, 1], [_e(3, 1), _e(4, _ulp(3, -1))], True),
    ("min one ulp below max / 3", [0, 1], [_e(3, _ulp(F32(7) / F32(3), -1)), _e(4, 7)], False),
    # (fl(7 / 3) * 3 = 7 - 2^-22 lies halfway between two floats and rounds to the even 7.0: 7 > 7 is false)
    ("min exactly fl(max / 3)", [0, 1], [_e(3, F32(7) / F32(3)), _e(4, 7)], True),
    ("min one ulp above fl(max / 3)", [0, 1], [_e(3, _ulp(F32(7) / F32(3), +1)), _e(4, 7)], True),
    # (min = 1 + 3 * 2^-23: 3 min = 3 + 4.5 * 2^-22 is a tie and rounds to the even 3 + 4 * 2^-22; max is the next float,
    # 3 + 5 * 2^-22; max / 3 = 1 + 3.33 * 2^-23 rounds to min, so min < max / 3 is false: ONLY the max test rejects)
    ("max one ulp above fl(3 min) while fl(max / 3) == min: only the max test rejects", [0, 1],
     [_e(3, float.fromhex("0x1.000006p+0")), _e(4, float.fromhex("0x1.80000ap+1"))], False),
    ("all distances exactly 0: max stays FLT_MIN, 0 < FLT_MIN / 3", [0, 1, 2], [_e(3, 0), _e(4, 0), _e(5, 0)], False),
    ("one distance 0, the others positive", [0, 1, 2], [_e(3, 0), _e(4, 1), _e(5, 1)], False),
    ("a view listed twice: one pair, not two (2 of 3 distinct)", [0, 1, 1], [_e(3, 2), _e(4, 2), _e(4, 2)], False),
    ("a view listed twice on a track of four: 3 distinct of 4", [0, 1, 1, 2], [_e(3, 2), _e(4, 2), _e(4, 2), _e(5, 2)], True),
]

# ---- component order: accepted points as (point id, [(view, polyline)]) in ascending point order -------------------------
COMPONENT_CASES = {
    "two components created in interleaved order": [
        (0, [(0, 5), (1, 5)]), (1, [(0, 1), (1, 1)]), (2, [(1, 5), (2, 5)]), (3, [(1, 1), (2, 0)])],
    "a later point merges two earlier components": [
        (0, [(0, 9), (1, 9)]), (1, [(0, 2), (1, 2)]), (2, [(2, 4), (3, 4)]), (5, [(0, 2), (1, 9)])],
    "a chain of merges more than two deep": [
        (0, [(0, 8), (1, 8)]), (1, [(0, 6), (1, 6)]), (2, [(0, 4), (1, 4)]), (3, [(0, 2), (1, 2)]),
        (4, [(1, 2), (2, 4)]), (5, [(1, 4), (2, 4)]), (6, [(1, 6), (2, 7)]), (7, [(2, 7), (0, 4)]), (8, [(0, 8), (2, 7)])],
}


def random_component_case(rng, n_views=4, n_pl=6):
    pts = []
    for pid in range(int(rng.integers(1, 12))):
        k = int(rng.integers(2, 5))
        pairs = {(int(rng.integers(0, n_views)), int(rng.integers(0, n_pl))) for _ in range(k)}
        if len(pairs) >= 2:
            pts.append((pid, sorted(pairs)))
    return pts


# ---- hand-built scenes for the device: straight and L-shaped polylines with real coordinates ------------------------------
def make_scene(n_views, width, height, polylines):
    """polylines: per view a list of vertex lists ([] or a single vertex: an invalid polyline)."""
    vpo, pvo, vtx, valid = [0], [0], [], []
    for v in range(n_views):
        for pl in polylines[v]:
            ok = len(pl) >= 2
            vtx.extend(pl if ok else [])
            pvo.append(len(vtx))
            valid.append(1 if ok else 0)
        vpo.append(len(valid))
    NP = len(valid)
    P = np.zeros((n_views, 16), np.float32)
    P[:, 0] = P[:, 5] = P[:, 10] = 1
    return {"n_views": n_views, "width": width, "height": height, "cam_P": P,
            "F": np.zeros((n_views, n_views, 9)), "F_valid": np.zeros((n_views, n_views), np.uint8),
            "view_pl_off": np.array(vpo, np.uint32), "pl_vtx_off": np.array(pvo, np.uint32),
            "vtx_xy": np.array(vtx if vtx else [[0, 0]], np.float32).reshape(-1, 2),
            "pl_start": np.arange(0, 2 * NP, 2, dtype=np.uint32), "pl_end": np.arange(1, 2 * NP + 1, 2, dtype=np.uint32),
            "pl_valid": np.array(valid, np.uint8)}


def make_seeds(tracks):
    """tracks: per point a list of (view, x, y)."""
    off, view, xy = [0], [], []
    for t in tracks:
        for (v, x, y) in t:
            view.append(v)
            xy.append((x, y))
        off.append(len(view))
    return (np.array(off, np.uint32), np.array(view, np.int32), np.array(xy if xy else [(0, 0)], np.float32).reshape(-1, 2))


def hline(y, x0, x1, n=2):
    return [(float(x), float(y)) for x in np.linspace(x0, x1, n)]


def rule_scene():
    """3 views of 200 x 150. Per view: 0 a horizontal line at y = 41; 1 an L (y = 81, then down at x = 151); 2 a horizontal
    line at y = 44 that ends at x = 60 (close to line 0: two polylines within 10 px for x < 60); 3 an invalid polyline;
    4 a short line inside the cell next to the boundary x = 100 (x 101..108 at y = 115); 5 a horizontal line ON the boundary
    row y = 130: every sample is dropped, no cell lists it, and a point 2 px from it finds nothing."""
    per_view = [hline(41, 10, 190, 6), [(20., 81.), (151., 81.), (151., 140.)], hline(44, 10, 60, 3), [(5., 5.)],
                hline(115, 101, 108, 2), hline(130, 20, 120, 3)]
    sc = make_scene(3, 200, 150, [per_view] * 3)
    T = [
        # accepted: distances 2, 2, 3 to line 0
        [(0, 100, 43), (1, 100, 43), (2, 100, 44)],
        # maxpl 2 in view 1 (lines 0 and 2 both within 10 px at x = 30)
        [(0, 100, 43), (1, 30, 42), (2, 100, 44)],
        # maxpl 0: nothing within 10 px anywhere
        [(0, 100, 61), (1, 100, 61), (2, 100, 61)],
        # 2 of 3 found: rejected by the share
        [(0, 100, 43), (1, 100, 43), (2, 100, 61)],
        # ratio exactly 3 (1 and 3 px below line 0): accepted; 3.5 px: rejected
        [(0, 100, 42), (1, 100, 44)],
        [(0, 100, 42), (1, 100, 44.5)],
        # 0.5 and 2 px
        [(0, 100, 41.5), (1, 100, 43)],
        # all distances exactly 0 (on the line): rejected through FLT_MIN
        [(0, 100, 41), (1, 120, 41)],
        # one distance 0
        [(0, 100, 41), (1, 100, 43), (2, 100, 43)],
        # a view listed twice: the last observation counts for both entries; 2 distinct of 3 -> rejected
        [(0, 100, 43), (1, 100, 61), (1, 100, 43)],
        # ... and of 4 with 3 distinct -> accepted; it names the L in all views: a second component
        [(0, 100, 83), (1, 100, 61), (1, 100, 83), (2, 100, 83)],
        # |S| = 1
        [(0, 100, 43)],
        # joins line 0 (views 0, 1) to the L (view 2): merges the two components
        [(0, 120, 43), (1, 120, 43), (2, 120, 79)],
        # on the boundary column x = 100: the window stops at the boundary, polyline 4 lies only in the cell beyond it;
        # next to it (x = 99.5) the full window finds it
        [(0, 100, 115), (1, 100, 115)],
        [(0, 99.5, 115), (1, 99.5, 115)],
        # on the boundary row y = 110 and on both
        [(0, 104, 110), (1, 104, 110)],
        [(0, 100, 110), (1, 100, 110)],
        # on and outside the image border
        [(0, 0, 41), (1, 200, 41)],
        [(0, -3, 41), (1, 100, 150)],
        # the L's vertical leg
        [(0, 153, 100), (1, 149, 100), (2, 153, 120)],
        # the line on the boundary row: 2 px away, found by no window
        [(0, 60, 132), (1, 60, 128)],
        # joins line 0 to the L once more, off the boundary column (point 12 sits on x = 120 and its window misses the L)
        [(0, 123, 43), (1, 123, 43), (2, 123, 79)],
    ]
    return sc, make_seeds(T)


def crowded_scene():
    """3 views of 64 x 48 with 70 polylines inside one 3 x 3 window (more than one batch of 64 candidates): 69 short lines
    more than 10 px away from the observation and, with the highest id, the only one within 10 px; view 2 has a second
    close one behind it (maxpl 2)."""
    far = [[(12. + 0.1 * k, 11.), (12. + 0.1 * k, 13.)] for k in range(69)]
    near = [[(22., 26.), (29., 26.)]]
    sc = make_scene(3, 64, 48, [far + near, far + near, far + near + [[(22., 27.), (29., 27.)]]])
    return sc, make_seeds([[(0, 25, 24), (1, 25, 23)], [(0, 25, 24), (2, 25, 24)], [(0, 25, 23), (0, 26, 24)]])


def boundary_sample_scene():
    """A polyline whose only samples in a cell fall on the boundary: a vertical line ON the column boundary x = 30 is listed
    nowhere; a line that crosses cell (4, 2) in less than one step on the boundary is listed only where a sample fell."""
    v = [[(30., 5.), (30., 40.)], [(40., 20.), (50., 20.)], [(5., 44.), (60., 44.)]]
    sc = make_scene(2, 64, 48, [v, v])
    return sc, make_seeds([[(0, 33, 20), (1, 33, 20)], [(0, 45, 22), (1, 45, 23)], [(0, 27, 43), (1, 33, 45)]])


def table_scene():
    """10 views x 8 two-vertex polylines: what the rule table's view and polyline ids index. The rows of the table become
    the tracks (coordinates unused: the per-entry results are fed to the rule directly)."""
    per_view = [hline(5 + 4 * k, 5, 55) for k in range(8)]
    sc = make_scene(10, 64, 48, [per_view] * 10)
    return sc, make_seeds([[(v, 1.0, 1.0) for v in row[1]] for row in RULE_TABLE])
