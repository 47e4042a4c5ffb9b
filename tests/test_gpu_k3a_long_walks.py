"""-m gpu: the walk service of the hypothesis stage (eg3d_k3a_engine.h k3a_walk_coop) on polylines whose epipolar walks
leave the lane-private head. The tiny and the small scene with every segment split into K collinear pieces (as
test_very_long_polylines_parity does): K = 3 — walks pass the head but fit one 64-segment pass; K = 14 — polylines of
more than 512 vertices, walks of several passes. Each with 64, 5 and 1 working lanes per wavefront (the service
is run by all 64 lanes whatever that number). The cloud, the flags and the counts must be the oracle's; the service's
own counters (read through the probe of the test-only engine variant, which runs the same K3a kernels) must show that the
long path ran."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from edgegraph3d_amd import api, build, host
from parity_util import compare_edgepoints

pytestmark = pytest.mark.gpu

_CACHE = {}


def _split_scene(cfg, K):
    s = host.Synth(cfg)
    sc = s.scene_np()
    pvo, vtx = sc["pl_vtx_off"], sc["vtx_xy"]
    new_off, new_vtx = [0], []
    for p in range(len(pvo) - 1):
        v = vtx[pvo[p]:pvo[p + 1]]
        if len(v) >= 2:
            for i in range(len(v) - 1):
                for k in range(K):
                    t = np.float32(k) / np.float32(K)
                    new_vtx.append(v[i] + (v[i + 1] - v[i]) * t)
            new_vtx.append(v[-1])
        new_off.append(len(new_vtx))
    sc["pl_vtx_off"] = np.asarray(new_off, np.uint32)
    sc["vtx_xy"] = np.asarray(new_vtx, np.float32).reshape(-1, 2)
    return s, sc, host.SceneArrays(sc)


def _case(cfg, K, form):
    """the scene and the oracle's answer (in the DLT form of the library under test): computed once, shared by the lanes cases"""
    key = (cfg, K, form)
    if key not in _CACHE:
        from oracle import binding as ob
        s, sc, sa = _split_scene(cfg, K)
        ref = ob.Oracle(C.byref(sa.c)).match(s.seeds, 0, s.n_seeds, nthreads=8)
        _CACHE[key] = (s, sc, sa, ref)
    return _CACHE[key]


@contextlib.contextmanager
def _library(path):
    old_env, old_lib = os.environ.get("EG3D_LIB"), api._LIB
    os.environ["EG3D_LIB"] = path
    api._LIB = None
    try:
        yield
    finally:
        api._LIB = old_lib
        if old_env is None:
            os.environ.pop("EG3D_LIB", None)
        else:
            os.environ["EG3D_LIB"] = old_env


def _same_as_oracle(ref, got, what):
    rep = compare_edgepoints(ref, got)
    assert rep["ok"] and rep["bitexact_X"] and rep["bitexact_xy"], (what, rep["msgs"][:3])
    assert got["flags"] == ref["flags"], (what, got["flags"], ref["flags"])
    assert got["n_hypotheses"] == ref["stats"]["n_hyp"] and got["n_chains"] == ref["stats"]["n_chains"], what


@pytest.mark.parametrize("lanes", ["64", "5", "1"])
@pytest.mark.parametrize("K", [3, 14])
@pytest.mark.parametrize("cfg", [0, 1])
def test_long_epipolar_walks_are_finished_by_the_wave(eg3d_form, monkeypatch, cfg, K, lanes):
    s, sc, sa, ref = _case(cfg, K, eg3d_form)
    if K == 14:
        assert np.diff(sc["pl_vtx_off"]).max() > 512
    if cfg == 0:
        assert ref["n_points"] > 100
    monkeypatch.setenv("EG3D_K3A_ENGINE_LANES", lanes)
    # the product library of this form
    ctx = api.Context(C.byref(sa.c))
    got = ctx.match_refpoints(s.seeds, 0, s.n_seeds)
    ctx.close()
    _same_as_oracle(ref, got, "product")
    # the same kernels in the engine variant (default DLT form only), which carries the probe
    assert os.path.exists(build.HIP_LIB_ENGINE), "variants/libeg3d_engine.so is not built (python -m edgegraph3d_amd.build)"
    with _library(build.HIP_LIB_ENGINE):
        ctx = api.Context(C.byref(sa.c))
        got = ctx.match_refpoints(s.seeds, 0, s.n_seeds)
        served, passes = ctx.probe_k3a_walks()
        ctx.close()
    if eg3d_form == 3:
        _same_as_oracle(ref, got, "variant")
    print("cfg %d K %d lanes %s: walks served %d, passes %d" % (cfg, K, lanes, served, passes))
    assert served > 0
    assert passes >= served
    if K == 14:
        assert passes > served
