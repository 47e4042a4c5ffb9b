"""SURVEY N4, the host statement of the device estimator (eg3d_host_estimate_fundamental, host/fundamental.cpp): the
arithmetic of csrc/eg3d_fund_core.h used in the plain way. Checked here without a GPU: the validity rule and the counts
against eg3d_host_estimate_F, reproducibility (run to run, and over the number of threads), and the geometric quality of
the matrices against the generator's cameras. tests/test_gpu_fundamental.py compares the device with it bit for bit."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from edgegraph3d_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def thinned_synth0():
    """Synth(0) thinned as in test_fmatrix.test_validity_rule_and_counts_match_the_oracle (some pairs fall below 10 common
    points), with a repeated view id inside one track and a view id outside the rig in another."""
    s = host.Synth(0)
    off, view, xy = s.seeds_np()
    V = s.n_views
    keep = np.ones(len(view), bool)
    rng = np.random.default_rng(5)
    for p in range(len(off) - 1):
        if p % 3:
            keep[rng.integers(off[p], off[p + 1])] = False
    new_off = np.zeros_like(off)
    new_off[1:] = np.cumsum([keep[off[p]:off[p + 1]].sum() for p in range(len(off) - 1)])
    view2, xy2 = view[keep].copy(), xy[keep].copy()
    assert new_off[1] - new_off[0] >= 2
    view2[new_off[0] + 1] = view2[new_off[0]]  # repeated view id: the later observation is the one used
    view2[new_off[2]] = V + 3                  # outside the rig: ignored
    view2[new_off[3]] = -1
    return V, new_off, view2, xy2


def test_validity_rule_and_counts_equal_those_of_estimate_F():
    V, off, view, xy = thinned_synth0()
    _, valid0, ncom0, _ = host.estimate_F(V, off, view, xy, estimate=False)
    F, valid, ncom, st = host.estimate_fundamental(V, (off, view, xy))
    assert np.array_equal(ncom, ncom0)
    assert np.array_equal(valid, valid0)  # (no pair of this scene fails)
    assert valid.any() and not valid.all()
    assert st["n_pairs_failed"] == 0 and st["n_pairs_valid"] == int(valid.sum())
    assert st["n_fits"] == 300 * int(valid.sum()) and st["n_common_total"] == int(ncom[valid != 0].sum())
    assert not np.any(F[valid == 0]) and np.all(np.isfinite(F))


_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from test_fundamental_host import thinned_synth0
from edgegraph3d_amd import host
V, off, view, xy = thinned_synth0()
F, valid, ncom, st = host.estimate_fundamental(V, (off, view, xy), rng_seed=11)
print(hashlib.sha256(F.tobytes() + valid.tobytes() + ncom.tobytes()).hexdigest())
"""


def test_same_bits_twice_and_on_one_thread():
    V, off, view, xy = thinned_synth0()
    a = host.estimate_fundamental(V, (off, view, xy), rng_seed=11)
    b = host.estimate_fundamental(V, (off, view, xy), rng_seed=11)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    want = hashlib.sha256(a[0].tobytes() + a[1].tobytes() + a[2].tobytes()).hexdigest()
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"))
    for threads in ("1", "3"):
        env = dict(os.environ, OMP_NUM_THREADS=threads)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
        assert out.split()[-1] == want, threads
    c = host.estimate_fundamental(V, (off, view, xy), rng_seed=12)
    assert not np.array_equal(a[0], c[0])  # (the seed is used)


@pytest.fixture(scope="module")
def c2():
    s = host.Synth(2)  # C2: 8 views, 2000 seeds, observation noise 0.4 px
    off, view, xy = s.seeds_np()
    return s, host.estimate_fundamental(s.n_views, (off, view, xy), rng_seed=7)


def worst_median_line_distance(s, F, valid):
    """test_fmatrix.test_estimate_agrees_with_the_cameras_geometrically: over the valid pairs, the largest median distance
    of the true projections (noise-free) from the epipolar lines of the estimate."""
    sc = s.scene_np()
    V = sc["n_views"]
    Xt = s.seed_truth()
    P = sc["cam_P"].reshape(V, 4, 4).astype(np.float64)
    Xh = np.concatenate([Xt, np.ones((len(Xt), 1))], 1)
    proj = []
    for v in range(V):
        q = Xh @ P[v].T
        proj.append(q[:, :2] / q[:, 2:3])

    def line_dist(Fm, a, b):
        h = np.concatenate([a, np.ones((len(a), 1))], 1)
        l = h @ Fm.reshape(3, 3).T
        return np.abs((l[:, 0] * b[:, 0] + l[:, 1] * b[:, 1] + l[:, 2])) / np.hypot(l[:, 0], l[:, 1])

    worst, checked = 0.0, 0
    wh = [sc["width"], sc["height"]]
    for i in range(V):
        for j in range(V):
            if i == j or not valid[i, j]:
                continue
            assert sc["F_valid"][i, j]
            inside = np.all((proj[i] > 0) & (proj[i] < wh) & (proj[j] > 0) & (proj[j] < wh), axis=1)
            assert np.median(line_dist(sc["F"][i, j], proj[i][inside], proj[j][inside])) < 1e-2
            worst = max(worst, float(np.median(line_dist(F[i, j], proj[i][inside], proj[j][inside]))))
            checked += 1
    assert checked >= V * (V - 1) // 2
    return worst


def test_estimate_agrees_with_the_cameras_geometrically(c2):
    s, (F, valid, ncom, st) = c2
    assert st["n_pairs_failed"] == 0
    worst = worst_median_line_distance(s, F, valid)
    print("worst median point-to-line distance: %.4f px" % worst)
    assert worst < 1.5, worst  # observation noise is 0.4 px; the analytic matrices give ~0


def test_agreement_with_estimate_F_is_reported(c2):
    """eg3d_host_estimate_F and this statement against the independent reference (tests/fundamental_ref.py) on C2, within its
    TOL, on every pair the reference decides (all 56: tests/test_fundamental_ref.py asserts that). The two normalise with
    hypot and with sqrt(dx*dx + dy*dy): a last-bit difference can flip a decision only where its margin is rounding noise,
    and a decided pair has margins of at least DELTA."""
    import fundamental_cases as fc
    import fundamental_ref as ref
    s, (F, valid, ncom, st) = c2
    case = fc.case("synth2")
    assert case["rng_seed"] == 7 and case["V"] == s.n_views
    off, view, xy = s.seeds_np()
    F0, valid0, ncom0, failed0 = host.estimate_F(s.n_views, off, view, xy, estimate=True, rng_seed=7)
    assert np.array_equal(valid, valid0) and np.array_equal(ncom, ncom0) and failed0 == 0
    Fr, valid_r, ncom_r, st_r, reports = fc.reference("synth2")
    assert np.array_equal(valid, valid_r) and np.array_equal(ncom, ncom_r)
    decided = [ij for ij, r in sorted(reports.items()) if ref.decided(r)]
    assert len(decided) == 56
    bad, worst = [], {"estimate_F": 0.0, "estimate_fundamental": 0.0}
    for ij in decided:
        for what, Fx in (("estimate_F", F0), ("estimate_fundamental", F)):
            d = ref.distance(Fx[ij], Fr[ij])
            worst[what] = max(worst[what], d)
            if d > ref.TOL:
                bad.append((what, ij, d, {m: reports[ij][m] for m in ("gap", "thr_gap", "mgap")}))
    equal_bits = sum(bool(np.array_equal(F[ij], F0[ij])) for ij in decided)
    print("worst distance from the reference: %s (pairs with equal bits in both: %d of %d)" % (worst, equal_bits, len(decided)))
    assert not bad, bad


def test_small_structs_and_bad_arguments_are_refused_before_anything_is_written():
    import ctypes as C
    from edgegraph3d_amd import _cdefs as D
    V, off, view, xy = thinned_synth0()
    L = host.lib()
    sd = D.Seeds(len(off) - 1, D.np_ptr(off, C.c_uint32), D.np_ptr(view, C.c_int32), D.np_ptr(xy, C.c_float))
    F = np.full((V, V, 9), 7.0)
    valid = np.full((V, V), 7, np.uint8)

    def call(n_views=V, seeds=C.byref(sd), pr_size=C.sizeof(D.FundParams), st_size=C.sizeof(D.FundStats)):
        pr, st = D.FundParams(pr_size), D.FundStats()
        st.struct_size = st_size
        rc = L.eg3d_host_estimate_fundamental(n_views, seeds, C.byref(pr), D.np_ptr(F, C.c_double), D.np_ptr(valid, C.c_uint8), None,
                                              C.byref(st))
        assert (F == 7.0).all() and (valid == 7).all()
        return rc

    assert call(pr_size=C.sizeof(D.FundParams) - 4) == -1 and call(st_size=C.sizeof(D.FundStats) - 4) == -1
    assert call(n_views=0) == -1 and call(seeds=None) == -1
    bad = off.copy()
    bad[2] = bad[3] + 1
    sd2 = D.Seeds(len(bad) - 1, D.np_ptr(bad, C.c_uint32), D.np_ptr(view, C.c_int32), D.np_ptr(xy, C.c_float))
    assert call(seeds=C.byref(sd2)) == -1
