"""Named inputs of the fundamental-matrix tests (tests/test_fundamental_ref.py on the CPU, tests/test_gpu_fundamental.py on the
device): V, tracks, iterations and seed. Data only; the expected results come from tests/fundamental_ref.py, computed once per
session (reference()).

WELL_POSED are compared with the reference (and, on the device, bit for bit with the host statement); every ordered pair of
every one of them is decided by the reference alone (tests/test_fundamental_ref.py asserts it). rectified() and
nan_majority() reach paths where an independent reference has no single answer: they are compared bit for bit with the host statement, plus one property each.
So are the `bounds` input of tests/test_gpu_fundamental.py (n = 10: recurring subsets and exact ties, the selection is tied by
construction) and its `hostile` scene (coincident or collinear observations: the null space of the design matrix is not
one-dimensional)."""
import time

import numpy as np

import fundamental_ref as ref


# ---- hand-made tracks ---------------------------------------------------------------------------------------------------------
def rig(n_views, n_points, seed):
    """n_points 3-D points in front of n_views cameras on an arc, projected to float32 pixels with 0.3 px noise: xy[v][p]"""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(-1.5, 1.5, (n_points, 2)), rng.uniform(5.0, 8.0, (n_points, 1))], 1)
    xy = np.zeros((n_views, n_points, 2), np.float32)
    for v in range(n_views):
        a = 0.12 * v
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        t = np.array([-0.6 * v, 0.05 * v, 0.1 * v])
        q = X @ R.T + t
        xy[v] = (np.stack([900 * q[:, 0] / q[:, 2] + 640, 900 * q[:, 1] / q[:, 2] + 480], 1)
                 + rng.normal(0, 0.3, (n_points, 2))).astype(np.float32)
    return xy


def tracks(per_point):
    """per_point: for every point the list of (view, x, y) in track order -> (trk_off, trk_view, trk_xy)"""
    off, view, xy = [0], [], []
    for obs in per_point:
        for v, x, y in obs:
            view.append(v)
            xy.append((x, y))
        off.append(len(view))
    return (np.asarray(off, np.uint32), np.asarray(view, np.int32), np.asarray(xy, np.float32).reshape(-1, 2))


def full_tracks(xy, views_of=None):
    V, n = xy.shape[:2]
    return tracks([[(v, xy[v, p, 0], xy[v, p, 1]) for v in (views_of(p) if views_of else range(V))] for p in range(n)])


# ---- well-posed cases -----------------------------------------------------------------------------------------------------------
def _boundary(c, seed):
    """3 views, c + 20 points. View 0 sees all of them, views 1 and 2 miss 20 scattered points each (not the same ones):
    n_common is c on (0, 1) and (0, 2), where view 0 holds the LONGER list and the short side has c entries, and c - 20 on
    (1, 2), whose lists are equally long. The holes make the ranks of the found lanes differ from their lane numbers."""
    n = c + 20
    xy = rig(3, n, seed)
    gone = np.random.default_rng(1000 + seed).permutation(n)[:40]
    miss = {1: set(gone[:20].tolist()), 2: set(gone[20:].tolist())}
    return dict(V=3, seeds=full_tracks(xy, lambda p: [v for v in range(3) if p not in miss.get(v, ())]), rng_seed=c,
                n_common={(0, 1): c, (0, 2): c, (1, 2): c - 20})


def _empty_views():
    """70 views (two wavefronts of view offsets); views 5, 68 and 69 have no observation at all, most pairs no common point,
    six pairs 20 to 40, one pair 5 (below the minimum). View 64 takes part in three pairs over different points."""
    per_point, want = [], {}
    for k, (a, b, n) in enumerate([(0, 1, 20), (3, 64, 25), (63, 64, 31), (64, 67, 33), (10, 66, 38), (2, 63, 40), (1, 7, 5)]):
        xy = rig(2, n, 40 + k)
        per_point += [[(a, xy[0, p, 0], xy[0, p, 1]), (b, xy[1, p, 0], xy[1, p, 1])] for p in range(n)]
        want[(a, b)] = n
    return dict(V=70, seeds=tracks(per_point), rng_seed=70, n_common=want)


def _stage32():
    """3 views whose pairs have 31, 32 and 33 common points: around stage_points = 32 in one call"""
    xy = rig(3, 96, 32)
    return dict(V=3, seeds=full_tracks(xy, lambda p: (0, 1) if p < 31 else (0, 2) if p < 63 else (1, 2)), rng_seed=32,
                n_common={(0, 1): 31, (0, 2): 32, (1, 2): 33})


def _stage_big():
    """two views, 1100 points: longer than the default staging area (1024), shorter than the largest (4096)"""
    return dict(V=2, seeds=full_tracks(rig(2, 1100, 11)), iterations=20, rng_seed=14, n_common={(0, 1): 1100})


def _v2():
    """the input of test_two_views_and_partial_waves_of_the_fit_kernel at 300 iterations: the refit is REJECTED on (0, 1)"""
    return dict(V=2, seeds=full_tracks(rig(2, 37, 2)), iterations=300, rng_seed=5, n_common={(0, 1): 37})


def _few_inliers():
    """12 points, 4 of them gross outliers (moved by up to 200 px in view 1): fewer than 8 inliers on both ordered pairs, so no refit
    runs and the matrix of the winning sample is the result (F_valid = 1)"""
    xy = rig(2, 12, 5)
    xy[1, [1, 4, 7, 10]] += np.array([[200, -120], [-150, 90], [60, 180], [-90, -200]], np.float32)
    return dict(V=2, seeds=full_tracks(xy), rng_seed=FEW_INLIERS_SEED, n_common={(0, 1): 12})


FEW_INLIERS_SEED = 32  # chosen with the reference: 7 inliers on both ordered pairs (seeds 0..31 leave 8 or 9 on one of them)

WELL_POSED = {
    "n63": lambda: _boundary(63, 63), "n64": lambda: _boundary(64, 64), "n65": lambda: _boundary(65, 65),
    "n127": lambda: _boundary(127, 127), "n128": lambda: _boundary(128, 128), "n129": lambda: _boundary(129, 129),
    "empty_views": _empty_views, "stage32": _stage32, "stage_big": _stage_big, "v2": _v2, "few_inliers": _few_inliers,
}


def _synth(config, rng_seed):
    from edgegraph3d_amd import host
    s = host.Synth(config)
    off, view, xy = s.seeds_np()
    return dict(V=s.n_views, seeds=(off.copy(), view.copy(), xy.copy()), rng_seed=rng_seed)


SCENES = {"synth0": lambda: _synth(0, 0), "synth2": lambda: _synth(2, 7)}


# ---- special paths ------------------------------------------------------------------------------------------------------------
RECTIFIED_F = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0]) / np.sqrt(2.0)


def rectified():
    """40 points on integer pixels, x2 = x1 + d (d an integer in 5..90), y2 = y1: every sample satisfies x2' F x1 = 0 exactly
    with F = RECTIFIED_F (up to sign). The medians are rounding noise, F33 is rounding noise (unit Frobenius norm instead of
    F33 = 1), the inlier threshold is its 1e-12 clamp and all 40 points are inliers."""
    rng = np.random.default_rng(6)
    x1, y1, d = rng.integers(100, 1100, 40), rng.integers(50, 900, 40), rng.integers(5, 91, 40)
    xy = np.stack([np.stack([x1, y1], 1), np.stack([x1 + d, y1], 1)]).astype(np.float32)
    return dict(V=2, seeds=full_tracks(xy), rng_seed=3)


def nan_majority(n, k, rng_seed):
    """two views, n points, the first k x-coordinates of view 1 NaN: a sample that avoids them (probability near 8e-4 at
    n = 21, k = 10) is the only non-degenerate one. With k < n - n // 2 its median is finite; from k = n - n // 2 on the
    n // 2-th smallest residual is 1e300 and the pair fails although it has non-degenerate fits."""
    xy = rig(2, n, 7)
    xy[1, :k, 0] = np.nan
    return dict(V=2, seeds=full_tracks(xy), iterations=6000, rng_seed=rng_seed)


# (n, k, rng_seed, the pairs are valid); the seeds leave each ordered pair at least 2 non-degenerate fits of its 6000
NAN_CASES = [(21, 10, 1, True), (21, 11, 1, False), (20, 9, 1, True), (20, 10, 3, False)]


def clean_samples(n, k, rng_seed, iterations=6000):
    """per ordered pair of a nan_majority input: how many of its samples avoid the first k points (from the reference's stream)"""
    out = {}
    for (i, j) in ((0, 1), (1, 0)):
        rng = ref.SplitMix64(ref.stream_seed(rng_seed, i * 2 + j))
        out[(i, j)] = sum(min(ref.draw_sample(rng, n)) >= k for _ in range(iterations))
    return out


# ---- the session's references -------------------------------------------------------------------------------------------------
_CASES, _REFS, SECONDS = {}, {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = (WELL_POSED.get(name) or SCENES[name])()
    return _CASES[name]


def kwargs(c):
    return {k: c[k] for k in ("iterations", "rng_seed") if k in c}


def reference(name):
    """fundamental_ref.estimate of a named case: (F, valid, n_common, counts, reports), computed once per session"""
    if name not in _REFS:
        c = case(name)
        t0 = time.perf_counter()
        _REFS[name] = ref.estimate(c["V"], c["seeds"], **kwargs(c))
        SECONDS[name] = time.perf_counter() - t0
    return _REFS[name]


def assert_close_to_reference(name, got, what):
    """`got` (F, valid, n_common, stats) of a native estimator on a named case against the reference: the counts equal, every
    pair decided, every matrix within TOL. Returns the worst distance and its pair."""
    F, valid, ncom, st = got[:4]
    F0, valid0, ncom0, st0, reports = reference(name)
    assert np.array_equal(ncom, ncom0), what
    assert np.array_equal(valid, valid0), what
    assert st["n_pairs_failed"] == st0["n_pairs_failed"] and st["n_pairs_valid"] == st0["n_pairs_valid"], what
    worst, at = 0.0, None
    for (i, j), r in sorted(reports.items()):
        assert ref.decided(r), (what, name, (i, j), r)
        if valid0[i, j]:
            d = ref.distance(F[i, j], F0[i, j])
            if d > worst:
                worst, at = d, (i, j)
    assert worst <= ref.TOL, (what, name, at, worst, reports[at])
    return worst, at
