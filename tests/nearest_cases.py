"""The cases the CPU and the GPU tests of the cloud-to-cloud nearest distances share (tests/test_nearest_host.py,
tests/test_gpu_nearest.py). A case is a dict: name, ref [m, 3] float32, ref_keep (uint8 [m] or None), X [n, 3] float32, keep
(uint8 [n] or None), cell, max_dist, thresholds. CASES is built once, seeded; reference(case) caches the brute force."""
import numpy as np

import nearest_ref

F = np.float32


def _case(name, ref, X, cell, max_dist, thresholds=(), ref_keep=None, keep=None):
    return {"name": name, "ref": np.ascontiguousarray(ref, F).reshape(-1, 3), "X": np.ascontiguousarray(X, F).reshape(-1, 3),
            "cell": float(F(cell)), "max_dist": float(F(max_dist)), "thresholds": tuple(float(F(t)) for t in thresholds),
            "ref_keep": None if ref_keep is None else np.ascontiguousarray(ref_keep, np.uint8),
            "keep": None if keep is None else np.ascontiguousarray(keep, np.uint8)}


def _lattice(cell, lo=-2, hi=2):
    """points on integer multiples of cell (computed in FP32), negative ones included"""
    k = np.arange(lo, hi + 1)
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3).astype(F)
    return (g * F(cell)).astype(F)


def _boundary_queries(ref, max_dist, rng, n_far=20):
    """around every reference point: at max_dist exactly along +-each axis (excluded by the strict rule), one ulp nearer
    (included), a small jitter; plus queries far away"""
    md = F(max_dist)
    inside = np.nextafter(md, F(0))
    out = []
    for a in range(3):
        for sgn in (F(1), F(-1)):
            for step in (md, inside):
                q = ref.copy()
                q[:, a] = (q[:, a] + sgn * step).astype(F)
                out.append(q)
    out.append((ref + rng.uniform(-0.6, 0.6, ref.shape).astype(F) * md).astype(F))
    span = float(np.abs(ref).max()) + 1.0
    out.append(rng.uniform(-40 * span, 40 * span, (n_far, 3)).astype(F))
    return np.concatenate(out).astype(F)


def _pair_case(cell, max_dist, seed):
    rng = np.random.default_rng(seed)
    ref = _lattice(cell)
    ref = np.concatenate([ref, ref[::7]])   # duplicated references: the tie goes to the smaller index
    X = _boundary_queries(ref[:50], max_dist, rng)
    return _case("pair_cell%g_md%g" % (cell, max_dist), ref, X, cell, max_dist, thresholds=(max_dist, 0.5 * max_dist))


def _build():
    rng = np.random.default_rng(1818)
    cases = []
    Q8 = rng.uniform(-1, 1, (40, 3))
    cases.append(_case("n_ref_0", np.zeros((0, 3)), Q8, 0.5, 0.5, thresholds=(0.25,)))
    cases.append(_case("n_ref_1", [[0.1, -0.2, 0.3]], np.concatenate([Q8, [[0.1, -0.2, 0.3]]]), 0.5, 0.5, thresholds=(0.25,)))
    cases.append(_case("n_ref_2", [[0.1, -0.2, 0.3], [-0.4, 0.2, 0.0]], Q8, 0.75, 0.5))
    cases.append(_case("n_queries_0", Q8, np.zeros((0, 3)), 0.5, 0.5, thresholds=(0.1,)))
    one_cell = rng.uniform(0.0, 0.2, (60, 3))
    cases.append(_case("one_cell", one_cell, rng.uniform(-0.3, 0.5, (120, 3)), 1.0, 0.25, thresholds=(0.1, 0.25)))
    lat = _lattice(0.25)
    cases.append(_case("lattice", lat, _boundary_queries(lat, 0.25, rng), 0.25, 0.25, thresholds=(0.25,)))
    # one reference alone: the 12 boundary queries come first — per axis and sign, at max_dist (excluded), one ulp nearer (included)
    for md in (0.25, 0.3):
        cases.append(_case("boundary_single_md%g" % md, np.zeros((1, 3)), _boundary_queries(np.zeros((1, 3), F), md, rng), md, md, thresholds=(md,)))
    # duplicates, and two distinct references equidistant from a query (0.25 and 0.75 are exact: both d2 are 0.0625)
    dup = np.array([[0.25, 0, 0], [0.75, 0, 0], [0.25, 0, 0], [0.75, 0, 0], [0, 0.5, 0], [0, 0.5, 0]], F)
    dq = np.array([[0.5, 0, 0], [0.25, 0, 0], [0.75, 0, 0], [0, 0.5, 0], [0, 0.25, 0.0]], F)
    cases.append(_case("ties", dup, dq, 0.5, 0.5))
    # a box of references; queries outside the bounding box by less and by more than max_dist
    box = rng.uniform(0, 1, (200, 3))
    faces = []   # past each face of the box, from the point that lies on it: by 0.05 (found) and by 0.15 (nothing)
    for a in range(3):
        for pick, sgn in ((np.argmax, 1.0), (np.argmin, -1.0)):
            for step in (0.05, 0.15):
                q = box[pick(box[:, a])].copy()
                q[a] += sgn * step
                faces.append(q)
    outq = np.concatenate([faces, box[:40] + [0, 0, 1.5], box[:40] - [3.0, 3.0, 3.0],
                           [[1.0 + 0.0999, 0.5, 0.5], [-0.0999, 0.5, 0.5], [1e30, 0, 0], [-1e30, 1e30, 3e38], [3e38, 3e38, 3e38]]])
    cases.append(_case("outside_box", box, outq, 0.125, 0.1, thresholds=(0.05, 0.1)))
    # NaN and +-inf on both sides, keep masks on both sides
    bad_ref = box.copy().astype(F)
    bad_ref[3, 0], bad_ref[10, 1], bad_ref[20, 2], bad_ref[30] = np.nan, np.inf, -np.inf, [np.nan, np.inf, 0]
    bad_q = rng.uniform(0, 1, (150, 3)).astype(F)
    bad_q[0, 2], bad_q[5, 0], bad_q[6, 1], bad_q[149] = np.nan, np.inf, -np.inf, [-np.inf, np.nan, np.nan]
    cases.append(_case("nonfinite", bad_ref, bad_q, 0.25, 0.2, thresholds=(0.1,)))
    rk = (rng.uniform(size=len(bad_ref)) < 0.6).astype(np.uint8)
    rk[3] = 0   # (a dropped non-finite reference counts as dropped)
    qk = (rng.uniform(size=len(bad_q)) < 0.7).astype(np.uint8)
    qk[0], qk[5] = 0, 1
    cases.append(_case("keep_masks", bad_ref, bad_q, 0.25, 0.2, thresholds=(0.1, 0.2), ref_keep=rk, keep=qk))
    cases.append(_case("keep_drops_all", box, bad_q, 0.25, 0.2, ref_keep=np.zeros(len(box), np.uint8), keep=np.zeros(len(bad_q), np.uint8)))
    # one cell holding 1000 points: longer than any chunk a lane or a wavefront takes at once; neighbours sparse
    # (the point (-1, -1, -1) is the origin, so [0.5, 1)^3 is one cell)
    crowd = np.concatenate([rng.uniform(0.55, 0.95, (1000, 3)), rng.uniform(-1, 2, (150, 3)), [[-1, -1, -1]]])
    cases.append(_case("crowded_cell", crowd, rng.uniform(0.3, 1.2, (130, 3)), 0.5, 0.5, thresholds=(0.05,)))
    # max_dist == cell (above), max_dist far below cell, eight thresholds, thresholds equal to max_dist
    cases.append(_case("md_far_below_cell", box, np.concatenate([box[:100] + rng.normal(0, 0.004, (100, 3)), Q8]), 2.0, 0.01,
                       thresholds=(0.01, 0.00125, 0.0025, 0.00375, 0.005, 0.00625, 0.0075, 0.00875)))
    R, Q = rng.uniform(-1, 1, (2000, 3)), rng.uniform(-1.1, 1.1, (3000, 3))
    cases.append(_case("random_3000x2000", R, Q, 0.125, 0.1, thresholds=(0.1, 0.05, 0.02)))
    for k, (cell, md) in enumerate(((0.25, 0.25), (0.1, 0.1), (0.3, 0.07), (1.0, 0.999))):
        cases.append(_pair_case(cell, md, 500 + k))
    return cases


CASES = _build()
IDS = [c["name"] for c in CASES]
_REF = {}


def reference(case):
    """(d2, nn, figures) of the brute force for `case`, computed once; callers must not change the arrays."""
    if case["name"] not in _REF:
        out = nearest_ref.nearest(case["ref"], case["X"], case["max_dist"], case["ref_keep"], case["keep"], case["thresholds"])
        for a in out[:2]:
            a.setflags(write=False)
        _REF[case["name"]] = out
    return _REF[case["name"]]


FIGURES = ("n_queries", "n_dropped", "n_nonfinite", "n_within", "n_below", "sum_q32")
D2_FIGURES = ("min_d2", "max_d2", "median_d2")


def assert_same(got, want, what):
    """(d2, nn, figures) against (d2, nn, figures): all d2 bits, all nn, every figure."""
    assert np.array_equal(np.asarray(got[0], F).view(np.uint32), np.asarray(want[0], F).view(np.uint32)), what + ": d2 bits"
    assert np.array_equal(got[1], want[1]), what + ": nn"
    for f in FIGURES:
        assert got[2][f] == want[2][f], (what, f, got[2][f], want[2][f])
    for f in D2_FIGURES:
        assert F(got[2][f]).view(np.uint32) == F(want[2][f]).view(np.uint32), (what, f, got[2][f], want[2][f])
