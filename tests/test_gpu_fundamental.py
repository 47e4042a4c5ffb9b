"""-m gpu: eg3d_estimate_fundamental (K12) against its host statement, eg3d_host_estimate_fundamental, BIT FOR BIT: F
(compared as uint64), F_valid, n_common, n_pairs_failed and n_fits_degenerate. The scenes are the synthetic ones and
hand-made tracks (no scene is needed: the call has no context). The reference of every input is computed once on the host
and shared by the two library forms the suite runs against; K12 does not depend on the DLT form.

Both sides of that comparison compile csrc/eg3d_fund_core.h, so it says nothing about the arithmetic. The named inputs of
tests/fundamental_cases.py are therefore also compared with the independent reference of tests/fundamental_ref.py, within its
TOL (tests/test_fundamental_ref.py does the same for the host statement and holds Synth(2)). The `bounds` input (n = 10:
recurring subsets, the selection is tied by construction) and the `hostile` scene (null spaces of more than one dimension)
stay bit-for-bit only: an independent reference has no single answer there."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cbuild
import fundamental_cases as fc
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host
from fundamental_cases import full_tracks, rig, tracks

pytestmark = pytest.mark.gpu

_REF = {}


def reference(name, V, seeds, **kw):
    """the host statement's result for a named input (computed once per session)"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _REF:
        kw.pop("fit_budget", None), kw.pop("stage_points", None)
        _REF[key] = host.estimate_fundamental(V, seeds, **kw)
    return _REF[key]


def assert_same(got, want):
    F, valid, ncom, st = got
    F0, valid0, ncom0, st0 = want
    assert np.array_equal(ncom, ncom0)
    assert np.array_equal(valid, valid0)
    assert np.array_equal(F.view(np.uint64), F0.view(np.uint64)), np.argwhere(F.view(np.uint64) != F0.view(np.uint64))[:8]
    for k in ("n_pairs_valid", "n_pairs_failed", "n_fits_degenerate", "n_fits", "n_common_total"):
        assert st[k] == st0[k], (k, st[k], st0[k])
    assert not np.isnan(F).any()


def check(name, V, seeds, **kw):
    got = api.estimate_fundamental(V, seeds, **kw)
    ref_kw = {k: v for k, v in kw.items() if k in ("iterations", "rng_seed")}
    assert_same(got, reference(name, V, seeds, **ref_kw))
    return got


def synth_tracks(config):
    s = host.Synth(config)
    off, view, xy = s.seeds_np()
    return s.n_views, (off.copy(), view.copy(), xy.copy())


# ---- scenes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [0, 2, 3], ids=["synth0", "c2", "c3"])
def test_scenes_with_default_parameters(config):
    V, seeds = synth_tracks(config)
    F, valid, ncom, st = check("synth%d" % config, V, seeds)
    assert st["n_pairs_valid"] > 0 and st["n_chunks"] >= 1


def test_one_view_has_no_pair():
    seeds = full_tracks(rig(1, 12, 1))
    F, valid, ncom, st = check("v1", 1, seeds)
    assert not F.any() and not valid.any() and not ncom.any()
    assert st["n_pairs_valid"] == st["n_pairs_failed"] == st["n_fits"] == st["n_chunks"] == 0
    # and no tracks at all
    empty = (np.zeros(1, np.uint32), np.zeros(0, np.int32), np.zeros((0, 2), np.float32))
    F, valid, ncom, st = check("v3_empty", 3, empty)
    assert not valid.any() and not ncom.any()


@pytest.mark.parametrize("iterations", [1, 63, 64, 65, 300])
def test_two_views_and_partial_waves_of_the_fit_kernel(iterations):
    seeds = full_tracks(rig(2, 37, 2))
    F, valid, ncom, st = check("v2", 2, seeds, iterations=iterations, rng_seed=5)
    assert ncom[0, 1] == ncom[1, 0] == 37 and st["n_fits"] == 2 * iterations
    if iterations >= 63:
        assert valid[0, 1] and valid[1, 0]


def test_boundaries_of_n_common_and_the_sample_stream_at_ten_points():
    """views (0, 1): exactly 9 common points (no matrix); (0, 2): exactly 10 (the n - 8 + (n == 8) term at n = 10; most
    draws of an 8-subset are rejected as duplicates, and the same subsets recur over 300 iterations: the tie rule of the
    selection decides); (1, 2): none."""
    xy = rig(3, 19, 3)
    seeds = full_tracks(xy, lambda p: (0, 1) if p < 9 else (0, 2))
    F, valid, ncom, st = check("bounds", 3, seeds, rng_seed=9)
    assert ncom[0, 1] == ncom[1, 0] == 9 and ncom[0, 2] == ncom[2, 0] == 10 and ncom[1, 2] == ncom[2, 1] == 0
    assert valid.tolist() == [[0, 0, 1], [0, 0, 0], [1, 0, 0]]
    assert st["n_fits"] == 600 and st["n_common_total"] == 20


def test_repeated_view_ids_and_view_ids_outside_the_rig():
    xy = rig(3, 30, 4)
    per_point = [[(v, xy[v, p, 0], xy[v, p, 1]) for v in range(3)] for p in range(30)]
    per_point[0].insert(0, (2, 11.0, 13.0))       # view 2 named twice: the LATER observation is the one used
    per_point[1].append((0, 700.0, 20.0))         # view 0 named twice, the later one is an outlier
    per_point[2] = [(1, 5.0, 5.0)] + per_point[2] + [(1, 6.0, 6.0), (1, 7.0, 7.0)]
    per_point[3].insert(1, (3, 1.0, 1.0))         # outside the rig: ignored
    per_point[4].append((-1, 1.0, 1.0))
    per_point[5] = [(7, 0.0, 0.0), (-5, 0.0, 0.0)]  # a track with nothing inside the rig
    per_point[6] = []
    seeds = tracks(per_point)
    F, valid, ncom, st = check("edge_tracks", 3, seeds, rng_seed=3)
    assert ncom[0, 1] == 28 and valid[0, 1]


def test_hostile_pairs_inside_a_good_scene():
    xy = rig(8, 40, 6)
    xy[2, :] = (333.25, 222.5)                                  # view 2: all observations coincident
    xy[3, :, 1] = 0.5 * xy[3, :, 0] + 100                       # view 3: all observations on one line
    xy[4, 7, 0] = np.nan                                        # view 4: a NaN coordinate
    xy[5, 9, 1] = np.inf                                        # view 5: an Inf coordinate
    xy[6, :, 0] = np.nan                                        # view 6: every sample of its pairs is degenerate
    seeds = full_tracks(xy)
    F, valid, ncom, st = check("hostile", 8, seeds, rng_seed=1)
    assert valid[0, 1] and valid[0, 7] and valid[7, 1]
    assert np.isfinite(F).all()
    assert not valid[6].any() and not valid[:, 6].any()
    assert st["n_pairs_failed"] == 14 and st["n_pairs_valid"] == 42


def test_chunking_gives_the_same_result():
    V, seeds = synth_tracks(2)
    one = check("synth2", V, seeds)
    n_pairs = one[3]["n_pairs_valid"] + one[3]["n_pairs_failed"]
    assert one[3]["n_chunks"] == 1 and n_pairs == 56
    for budget, chunks in ((300, n_pairs), (1, n_pairs), (19 * 300, 3), (19 * 300 + 299, 3)):
        got = check("synth2", V, seeds, fit_budget=budget)
        assert got[3]["n_chunks"] == chunks, (budget, got[3]["n_chunks"])
        assert np.array_equal(got[0].view(np.uint64), one[0].view(np.uint64))


def test_staging_and_the_selection_path():
    V, seeds = synth_tracks(2)
    one = check("synth2", V, seeds)
    assert one[2][one[1] != 0].min() > 16
    mem = check("synth2", V, seeds, stage_points=16)  # every pair is longer than the staging area: read from memory
    assert np.array_equal(mem[0].view(np.uint64), one[0].view(np.uint64))
    # the count path is the one that ran: a handful of exact medians per pair, not one per iteration
    assert 0 < one[3]["n_exact_medians"] < 300 * 56
    assert one[3]["n_exact_medians"] == mem[3]["n_exact_medians"]
    print("exact medians per pair: %.1f" % (one[3]["n_exact_medians"] / 56.0))


# ---- the named cases: the independent reference, and the boundaries of the kernels -------------------------------------------
def check_case(name, **kw):
    c = fc.case(name)
    return check("case_" + name, c["V"], c["seeds"], **fc.kwargs(c), **kw)


@pytest.mark.parametrize("name", list(fc.WELL_POSED) + ["synth0"])
def test_cases_equal_the_independent_reference_and_the_host_bits(name):
    """n63 .. n129: the wavefront boundaries of the ballot ranks (common points, inliers) and of the strides of 64, with
    unequal lists (view i the longer one) and equal ones; empty_views: views without observations among 70; stage32,
    stage_big: around the staging area; v2 / n65: the refit rejected / kept; few_inliers: no refit at all."""
    got = check_case(name)
    for (i, j), n in fc.case(name).get("n_common", {}).items():
        assert got[2][i, j] == got[2][j, i] == n
    worst, at = fc.assert_close_to_reference(name, got, "device")
    print("%s: worst max|F - F_ref| / max|F_ref| = %.3g at %s" % (name, worst, at))


def test_staging_boundary_31_32_33_points_around_a_staging_area_of_32():
    one = check_case("stage32")
    assert sorted({int(n) for n in one[2].ravel()}) == [0, 31, 32, 33] and one[3]["n_pairs_valid"] == 6
    for stage_points in (32, 31, 33):
        got = check_case("stage32", stage_points=stage_points)
        assert np.array_equal(got[0].view(np.uint64), one[0].view(np.uint64)), stage_points


@pytest.mark.parametrize("stage_points", [4096, 5000])
def test_the_largest_staging_area(stage_points):
    """1100 points: read from memory with the default staging area (1024), staged with the largest one (4096 points, 64 KB
    of dynamic LDS); a larger request is clamped to it"""
    one = check_case("stage_big")
    assert one[2][0, 1] == 1100 and one[1][0, 1] and one[1][1, 0]
    got = check_case("stage_big", stage_points=stage_points)
    assert np.array_equal(got[0].view(np.uint64), one[0].view(np.uint64))
    assert got[3]["n_exact_medians"] == one[3]["n_exact_medians"]


def test_rectified_pair_frobenius_branch_and_threshold_clamp():
    from test_fundamental_ref import rectified_properties
    c = fc.rectified()
    F, valid, ncom, st = check("rectified", c["V"], c["seeds"], **fc.kwargs(c))
    rectified_properties(F, valid)


@pytest.mark.parametrize("n,k,rng_seed,ok", fc.NAN_CASES)
def test_median_among_a_non_finite_majority(n, k, rng_seed, ok):
    """a handful of non-degenerate fits among 6000; their median is finite (k NaN points below n - n // 2) or 1e300 (from
    there on: no matrix, although fits exist). The count path runs with best == 1e300, the exact median over keys that are
    mostly 1e300."""
    c = fc.nan_majority(n, k, rng_seed)
    F, valid, ncom, st = check("nan_%d_%d" % (n, k), c["V"], c["seeds"], **fc.kwargs(c))
    assert valid.tolist() == ([[0, 1], [1, 0]] if ok else [[0, 0], [0, 0]])
    assert st["n_fits_degenerate"] == 12000 - sum(fc.clean_samples(n, k, rng_seed).values())
    assert st["n_pairs_failed"] == (0 if ok else 2) and (st["n_exact_medians"] >= 2) == ok


def test_two_calls_give_equal_bits_and_all_memory_comes_back():
    live = api.lib().eg3d_test_live_device_bytes
    live.restype = C.c_int64
    before = live()
    V, seeds = synth_tracks(0)
    a = api.estimate_fundamental(V, seeds, rng_seed=21)
    assert live() == before
    again = api.estimate_fundamental(V, seeds, rng_seed=21)  # the same arguments: the same bits
    assert live() == before
    b = api.estimate_fundamental(V, seeds, rng_seed=21, fit_budget=600)
    assert live() == before
    for other in (again, b):
        assert np.array_equal(a[0].view(np.uint64), other[0].view(np.uint64))
        assert np.array_equal(a[1], other[1]) and np.array_equal(a[2], other[2])
    assert {k: v for k, v in a[3].items() if not k.startswith("ms_")} == {k: v for k, v in again[3].items() if not k.startswith("ms_")}
    assert_same(a, reference("synth0", V, seeds, rng_seed=21))


def test_refusals_leave_the_outputs_untouched():
    L = api.lib()
    V, (off, view, xy) = synth_tracks(0)
    sd = D.Seeds(len(off) - 1, D.np_ptr(off, C.c_uint32), D.np_ptr(view, C.c_int32), D.np_ptr(xy, C.c_float))
    F = np.full((V, V, 9), 7.0)
    valid = np.full((V, V), 7, np.uint8)
    ncom = np.full((V, V), 7, np.uint32)

    def call(n_views=V, seeds=C.byref(sd), pr_size=C.sizeof(D.FundParams), st_size=C.sizeof(D.FundStats), Fp=None):
        pr = D.FundParams(pr_size)
        st = D.FundStats()
        st.struct_size = st_size
        st.n_fits = 77
        rc = L.eg3d_estimate_fundamental(0, n_views, seeds, C.byref(pr), D.np_ptr(F, C.c_double) if Fp is None else Fp,
                                         D.np_ptr(valid, C.c_uint8), D.np_ptr(ncom, C.c_uint32), C.byref(st))
        assert st.n_fits == 77
        assert (F == 7.0).all() and (valid == 7).all() and (ncom == 7).all()
        return rc

    assert call(st_size=C.sizeof(D.FundStats) - 4) == -1 and b"struct_size" in L.eg3d_last_error()
    assert call(pr_size=C.sizeof(D.FundParams) - 4) == -1 and b"struct_size" in L.eg3d_last_error()
    assert call(Fp=C.POINTER(C.c_double)()) == -1
    assert call(n_views=0) == -1 and call(n_views=-3) == -1
    assert call(seeds=None) == -1
    bad = off.copy()
    bad[2] = bad[3] + 1  # offsets that do not ascend
    sd2 = D.Seeds(len(bad) - 1, D.np_ptr(bad, C.c_uint32), D.np_ptr(view, C.c_int32), D.np_ptr(xy, C.c_float))
    assert call(seeds=C.byref(sd2)) == -1
    # the host statement refuses the same
    with pytest.raises(RuntimeError):
        host.estimate_fundamental(0, (off, view, xy))
    with pytest.raises(RuntimeError):
        host.estimate_fundamental(V, (bad, view, xy))


def test_estimate_agrees_with_the_cameras_geometrically():
    from test_fundamental_host import worst_median_line_distance
    s = host.Synth(2)
    F, valid, ncom, st = api.estimate_fundamental(s.n_views, s.seeds, rng_seed=7)
    assert st["n_pairs_failed"] == 0
    worst = worst_median_line_distance(s, F, valid)
    assert worst < 1.5, worst  # observation noise is 0.4 px; the analytic matrices give ~0


def test_end_to_end_the_example_and_python_report_the_same_cloud(tmp_path):
    """The device's matrices in the scene of Synth(2) -> match_refpoints, against examples/edge_matcher_refpoints.cpp run
    with --estimate-F --estimate-F-device on the files of the same scene (the example links the default library: the
    Python side of this comparison uses it too, whichever form the test runs under)."""
    import forms
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path, lib=cbuild.DEFAULT_LIB)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "2", d])
    out = subprocess.run([exe, d + "/input.json", d + "/plgs.bin", d + "/out.json", "--estimate-F", "--estimate-F-device"],
                         capture_output=True, text=True, timeout=300, env=dict(os.environ, EG3D_LIB=""))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "on the device" in out.stdout
    m = re.search(r"-> (\d+) edge-points \((\d+) observations\)", out.stdout)
    assert m, out.stdout
    s = host.Synth(2)
    F, valid, ncom, st = api.estimate_fundamental(s.n_views, s.seeds, rng_seed=0xE63D2018)
    off, view, xy = s.seeds_np()
    _, rule, _, _ = host.estimate_F(s.n_views, off, view, xy, estimate=False)
    sc = s.scene_np()
    sc["F"] = F
    sc["F_valid"] = (valid & rule).astype(np.uint8)
    sa = host.SceneArrays(sc)
    with forms.product_form(3):
        ctx = api.Context(C.byref(sa.c))
        got = ctx.match_refpoints(s.seeds)
        ctx.close()
    assert got["n_points"] > 0
    assert (int(m.group(1)), int(m.group(2))) == (got["n_points"], got["n_obs"]), out.stdout
