"""CPU tests of the fundamental-matrix estimator against an INDEPENDENT reference. tests/test_gpu_fundamental.py compares the
device with the host statement (eg3d_host_estimate_fundamental) bit for bit, but both compile csrc/eg3d_fund_core.h: a
mistake in the stream, the normalisation, the row layout, the eigenvector, the rank-2 step, the denormalisation, the
residual, the median index, the selection, the threshold or the refit's rule would be the same on both sides. Here the host
statement is compared with tests/fundamental_ref.py (NumPy, other numerical routes), after that file is pinned itself: its
stream against the published SplitMix64 vectors, its fit against the analytic matrix of known cameras. The inputs are those
of tests/fundamental_cases.py, which the device tests share."""
import numpy as np
import pytest

import fundamental_cases as fc
import fundamental_ref as ref
from edgegraph3d_amd import host

COMPARED = list(fc.WELL_POSED) + list(fc.SCENES)


# ---- the reference itself -----------------------------------------------------------------------------------------------------
def test_splitmix64_published_vectors():
    rng = ref.SplitMix64(1234567)
    assert [rng.next() for _ in range(5)] == [6457827717110365317, 3203168211198807973, 9817491932198370423,
                                              4593380528125082431, 16408922859458223821]


def test_stream_seed_and_the_redraw_of_a_duplicate():
    assert ref.stream_seed(0, 0) == 0x9E3779B97F4A7C15
    assert ref.stream_seed(5, 2) == 5 ^ ((3 * 0x9E3779B97F4A7C15) % 2 ** 64)
    assert ref.stream_seed(2 ** 64 - 1, 6) == (2 ** 64 - 1) ^ ((7 * 0x9E3779B97F4A7C15) % 2 ** 64)
    # the published vectors end in 7, 3, 3, 1, 1: below(10) repeats 3 and 1, both are drawn again
    s = ref.draw_sample(ref.SplitMix64(1234567), 10)
    assert s[:3] == [7, 3, 1] and len(set(s)) == 8 and all(0 <= k < 10 for k in s)
    rng = ref.SplitMix64(99)
    assert sorted(ref.draw_sample(rng, 8)) == list(range(8))


def test_common_points_last_observation_wins_and_foreign_ids_are_ignored():
    per_point = [
        [(0, 1.0, 2.0), (1, 3.0, 4.0)],
        [(1, 5.0, 6.0), (0, 7.0, 8.0), (1, 9.0, 10.0)],      # view 1 twice: (9, 10) is used
        [(0, 1.5, 2.5), (2, 0.0, 0.0), (-1, 0.0, 0.0)],      # ids outside a rig of 2: ignored; not seen from view 1
        [],
        [(1, 11.0, 12.0), (0, 13.0, 14.0), (0, 15.0, 16.0)],  # view 0 twice
    ]
    seeds = fc.tracks(per_point)
    x1, y1, x2, y2 = ref.correspondences(ref.observations(2, seeds), 0, 1)
    assert x1.tolist() == [1.0, 7.0, 15.0] and y1.tolist() == [2.0, 8.0, 16.0]
    assert x2.tolist() == [3.0, 9.0, 11.0] and y2.tolist() == [4.0, 10.0, 12.0]
    _, _, ncom, _, _ = ref.estimate(2, seeds)
    assert ncom.tolist() == [[0, 3], [3, 0]]
    assert np.array_equal(host.estimate_fundamental(2, seeds)[2], ncom)


def _analytic_pair(n, seed):
    """noise-free float64 projections of n points through K [I | 0] and K [R | t], and F = K^-T [t]x R K^-1 (x2' F x1 = 0)"""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(-1.5, 1.5, (n, 2)), rng.uniform(5.0, 8.0, (n, 1))], 1)
    K = np.array([[900.0, 0, 640], [0, 900, 480], [0, 0, 1]])
    a = 0.12
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([-0.6, 0.05, 0.1])
    q1, q2 = X @ K.T, (X @ R.T + t) @ K.T
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    Fa = Ki.T @ tx @ R @ Ki
    return q1[:, 0] / q1[:, 2], q1[:, 1] / q1[:, 2], q2[:, 0] / q2[:, 2], q2[:, 1] / q2[:, 2], Fa / Fa[2, 2]


# A fit of exact data errs by about the rounding unit (1.1e-16) times the condition of its normalised design matrix, largest
# to second smallest singular value: below 1e3 for 40 spread points, up to about 1e5 for an unlucky sample of 8. Ten times
# that is the bound. A transposed matrix, swapped normalisations or another row layout are wrong by the size of the matrix.
ANCHOR_ALL, ANCHOR_SAMPLE = 1e-12, 1e-10


def test_reference_fit_equals_the_analytic_matrix_of_known_cameras():
    x1, y1, x2, y2, Fa = _analytic_pair(40, 1)
    F, ok, frob = ref.fit(x1, y1, x2, y2)
    assert ok and not frob
    d_all = ref.distance(F, Fa)
    rng = ref.SplitMix64(7)
    idx = np.array([ref.draw_sample(rng, 40) for _ in range(50)])
    Fs, ok, frob = ref.fit(x1[idx], y1[idx], x2[idx], y2[idx])
    assert ok.all() and not frob.any()
    d_sample = max(ref.distance(f, Fa) for f in Fs)
    # the ordered pair the other way round is the transpose
    Ft, _, _ = ref.fit(x2, y2, x1, y1)
    d_t = ref.distance(Ft, Fa.T / Fa.T[2, 2])
    # the whole estimator on exact data: every median is rounding noise, whichever sample wins is right
    Fl, rep = ref.lmeds(x1, y1, x2, y2, 100, 11)
    d_lmeds = ref.distance(Fl, Fa)
    print("analytic anchor: all points %.3g, transposed %.3g, worst of 50 samples %.3g, lmeds %.3g" % (d_all, d_t, d_sample, d_lmeds))
    assert d_all <= ANCHOR_ALL and d_t <= ANCHOR_ALL
    assert d_sample <= ANCHOR_SAMPLE and d_lmeds <= ANCHOR_SAMPLE
    assert ref.residuals(Fa, x1, y1, x2, y2).max() < 1e-18  # (and the residual is that of x2' F x1 = 0, not of x1' F x2)
    assert ref.residuals(Fa.T, x1, y1, x2, y2).max() > 1.0


def test_reference_residual_is_the_larger_distance_and_the_median_the_upper_one():
    F = np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])  # rectified: the lines are y = const in both images
    r = ref.residuals(F, np.array([10.0, 20.0]), np.array([5.0, 7.0]), np.array([30.0, 40.0]), np.array([8.0, 7.0]))
    assert r.tolist() == [9.0, 0.0]
    Fs = np.array([[0.0, 0, 0], [0, 0, -2], [0, 1, 0]])  # distances 11 in image 1 and 11 / 2 in image 2 for y1 = 5, y2 = 8
    assert ref.residuals(Fs, np.array([10.0]), np.array([5.0]), np.array([30.0]), np.array([8.0])).tolist() == [121.0]
    assert ref.residuals(F, np.array([np.nan]), np.array([5.0]), np.array([30.0]), np.array([8.0])).tolist() == [1e300]
    assert ref.median(np.array([4.0, 1.0, 3.0, 2.0])) == 3.0 and ref.median(np.array([5.0, 1.0, 3.0])) == 3.0
    assert ref.inlier_threshold(1e-27, 40) == 1e-12
    assert ref.inlier_threshold(0.04, 18) == pytest.approx((2.5 * 1.4826 * 1.5 * 0.2) ** 2, rel=1e-15)


# ---- the host statement against the reference ---------------------------------------------------------------------------------
_HOST = {}


def host_result(name):
    if name not in _HOST:
        c = fc.case(name)
        _HOST[name] = host.estimate_fundamental(c["V"], c["seeds"], **fc.kwargs(c))
    return _HOST[name]


@pytest.mark.parametrize("name", COMPARED)
def test_every_pair_is_decided_by_the_reference_alone(name):
    """No pair is left out of the comparison: the seeds of the cases were chosen so that every decision of every pair (the
    winner, every inlier, the refit's acceptance) has a relative margin of at least DELTA."""
    reports = fc.reference(name)[4]
    assert reports
    least = {m: min((r[m], ij) for ij, r in reports.items()) for m in ("gap", "thr_gap", "mgap")}
    print("%s: %d pairs, reference %.2f s, smallest margins %s" % (name, len(reports), fc.SECONDS[name], least))
    for ij, r in reports.items():
        assert ref.decided(r), (ij, r)
    assert min(v[0] for v in least.values()) >= ref.DELTA


@pytest.mark.parametrize("name", COMPARED)
def test_host_statement_equals_the_reference(name):
    c = fc.case(name)
    got = host_result(name)
    for (i, j), n in c.get("n_common", {}).items():
        assert got[2][i, j] == got[2][j, i] == n, (i, j)
    worst, at = fc.assert_close_to_reference(name, got, "host statement")
    print("%s: worst max|F - F_ref| / max|F_ref| = %.3g at %s" % (name, worst, at))
    assert got[3]["n_fits_degenerate"] == sum(r["n_degenerate"] for r in fc.reference(name)[4].values())


@pytest.mark.parametrize("c", [63, 64, 65, 127, 128, 129])
def test_boundary_rigs_have_the_list_lengths_the_device_paths_need(c):
    """On (0, 1) and (0, 2) view 0 holds the longer list (the device walks the list of view j and searches in view i's);
    on (1, 2) the lists are equally long."""
    per_view = ref.observations(3, fc.case("n%d" % c)["seeds"])
    assert [len(v) for v in per_view] == [c + 20, c, c]
    ncom = fc.reference("n%d" % c)[2]
    assert ncom[0, 1] == ncom[0, 2] == c and ncom[1, 2] == c - 20
    first = sorted(per_view[0].keys() & per_view[1].keys())[:64]
    assert first != list(range(64))  # (holes: a found lane's rank is not its lane number)


def test_empty_views_case_has_views_without_any_observation():
    c = fc.case("empty_views")
    per_view = ref.observations(70, c["seeds"])
    assert not per_view[5] and not per_view[68] and not per_view[69]
    F, valid, ncom, st, reports = fc.reference("empty_views")
    assert len(reports) == 12 and st["n_pairs_valid"] == 12
    assert sorted(int(n) for n in ncom[ncom > 0]) == sorted([20, 25, 31, 33, 38, 40, 5] * 2)
    got = host_result("empty_views")
    assert not got[1][5].any() and not got[1][:, 69].any() and not got[0][68].any()


def test_both_refit_outcomes_are_covered():
    rejected = fc.reference("v2")[4][(0, 1)]
    assert rejected["refit_ran"] and not rejected["refit_kept"] and rejected["n_in"] == 33
    kept = fc.reference("n65")[4][(0, 1)]
    assert kept["refit_ran"] and kept["refit_kept"] and kept["n_in"] == 65


def test_few_inliers_no_refit_and_still_a_matrix():
    F, valid, ncom, st, reports = fc.reference("few_inliers")
    for ij in ((0, 1), (1, 0)):
        assert reports[ij]["n_in"] == 7 and not reports[ij]["refit_ran"] and valid[ij]
    got = host_result("few_inliers")
    assert got[1][0, 1] and got[1][1, 0] and got[3]["n_pairs_failed"] == 0


# ---- special paths: properties of the host statement --------------------------------------------------------------------------
# the largest deviation of the host statement's matrix from +-RECTIFIED_F measured on a CPU is 2.33e-13 (ordered pair
# (1, 0)); the bound is 100 times that
RECTIFIED_BOUND = 2.33e-11


def rectified_properties(F, valid):
    """asserted of the host statement here and of the device in tests/test_gpu_fundamental.py"""
    c = fc.rectified()
    per_view = ref.observations(2, c["seeds"])
    worst = 0.0
    for (i, j) in ((0, 1), (1, 0)):
        assert valid[i, j]
        f = F[i, j]
        assert abs(np.sqrt((f * f).sum()) - 1.0) < 1e-15   # unit Frobenius norm: the branch of a tiny F33
        assert abs(f[8]) <= 1e-12
        worst = max(worst, min(np.max(np.abs(f - fc.RECTIFIED_F)), np.max(np.abs(f + fc.RECTIFIED_F))))
        res = ref.residuals(f.reshape(3, 3), *ref.correspondences(per_view, i, j))
        assert res.max() <= 1e-12 and ref.inlier_threshold(float(ref.median(res)), 40) == 1e-12  # the clamp: all 40 are inliers
    assert worst <= RECTIFIED_BOUND, worst
    return worst


def test_rectified_pair_takes_the_frobenius_branch_and_the_threshold_clamp():
    c = fc.rectified()
    F, valid, ncom, st = host.estimate_fundamental(c["V"], c["seeds"], **fc.kwargs(c))
    assert ncom[0, 1] == 40 and st["n_fits_degenerate"] == 0
    print("rectified pair: largest deviation from +-RECTIFIED_F %.3g" % rectified_properties(F, valid))


@pytest.mark.parametrize("n,k,rng_seed,ok", fc.NAN_CASES)
def test_median_among_a_non_finite_majority(n, k, rng_seed, ok):
    clean = fc.clean_samples(n, k, rng_seed)
    assert min(clean.values()) >= 2, clean  # (every pair has fits to select among: a failure is the median's, not theirs)
    c = fc.nan_majority(n, k, rng_seed)
    F, valid, ncom, st = host.estimate_fundamental(c["V"], c["seeds"], **fc.kwargs(c))
    assert ncom[0, 1] == n and st["n_fits"] == 12000
    assert st["n_fits_degenerate"] == 12000 - sum(clean.values())
    assert valid.tolist() == ([[0, 1], [1, 0]] if ok else [[0, 0], [0, 0]])
    assert st["n_pairs_failed"] == (0 if ok else 2) and np.isfinite(F).all() and bool(F.any()) == ok
