"""-m gpu: the retries of stage B (eg3d_api_match_stage_b.hip run_stage_b), alone and all in one call. A launch of the expand
stage can be answered in five ways: K2's hit buffer was too small (EG3D_HITS_CAP0), the hypothesis arena overflowed
(EG3D_ARENA_CAP0), chains outgrew their working slices (EG3D_CHAIN_CAP0 / EG3D_POOL_CAP0), a few-views build refused a
solve (EG3D_K3B_ASSUME_SHORT: test_gpu_parity.py), and the staging area the finished chains are packed into was too small
(EG3D_STAGE_CAP0). Every one of them repeats work whose first attempt has already counted bytes and packed results, so the
property is the same each time: the call's cloud, counts and byte counter are BYTE FOR BYTE those of a call that met none
of them (and that one is compared with the oracle), in the host arrays and in the device view alike."""
import numpy as np
import pytest

from edgegraph3d_amd import api, host
from parity_util import compare_edgepoints

pytestmark = pytest.mark.gpu

ARRAYS = ("X", "obs_off", "obs_view", "obs_pl", "obs_seg", "obs_xy", "key")
COUNTS = ("n_points", "n_obs", "n_tasks", "n_hypotheses", "n_chains", "flags")


def _oracle(scene):
    from oracle import binding as ob
    return ob.Oracle(scene)


def _same(a, b, what):
    for k in COUNTS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ARRAYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)
    assert a["times"]["bytes_algorithmic"] == b["times"]["bytes_algorithmic"], what


_BASE = {}


def _base(rows):
    """host.Synth(1) (the suite's smallest scene that still produces chains) and its clouds of both paths from a context
    that no knob touches, uncut, each compared bit-exactly with the oracle: computed once per DLT form, shared read-only.
    Call it BEFORE setting a knob."""
    if rows not in _BASE:
        s = host.Synth(1)
        sets = s.polyline_sets()
        ctx = api.Context(s.scene)
        ctx.upload_seeds(s.seeds)
        ctx.set_pipelining(1, 0)
        clouds = {"seeds": ctx.match_resident(0, s.n_seeds), "sets": ctx.match_polyline_sets(*sets)}
        ctx.close()
        o = _oracle(s.scene)
        refs = {"seeds": o.match(s.seeds, 0, s.n_seeds, nthreads=8), "sets": o.match_polyline_sets(*sets, nthreads=8)}
        for path in clouds:
            rep = compare_edgepoints(refs[path], clouds[path])
            assert rep["ok"] and rep["bitexact_X"] and rep["bitexact_xy"], (path, rep["msgs"][:3])
            assert clouds[path]["n_chains"] > 0 and clouds[path]["n_points"] > 1
        _BASE[rows] = (s, sets, clouds)
    return _BASE[rows]


def _call(ctx, s, sets, path, device_only):
    """One call of `path`; a device-only call's result is its counts and times with the arrays of the device view."""
    if path == "seeds":
        d = ctx.match_resident(0, s.n_seeds, device_only=device_only)
    else:
        d = ctx.match_polyline_sets(*sets, device_only=device_only)
    if device_only:
        dev = ctx.fetch_device_output()
        assert dev["n_points"] == d["n_points"] and dev["n_obs"] == d["n_obs"]
        d.update({k: dev[k] for k in ARRAYS})
    return d


@pytest.mark.parametrize("path", ["seeds", "sets"])
def test_a_staging_area_that_is_too_small_is_sized_for_the_need_and_the_launch_repeated(eg3d_form, monkeypatch, capfd, path):
    """EG3D_STAGE_CAP0=1: the first expand launch of a context packs into a staging area of one point, so its chains are
    counted but not packed; the host sizes the area for what the output scans report, takes the launch's share of the
    byte counter back and repeats the launch (the trace says so). Whether the context's first call is a host call or a
    device-only one: the same cloud, counts and byte counter as without the knob, and the call after it — of the other
    kind — needs no second launch, because the need was learned."""
    s, sets, clouds = _base(eg3d_form)
    monkeypatch.setenv("EG3D_STAGE_CAP0", "1")
    monkeypatch.setenv("EG3D_TRACE_ARENA", "1")
    for first_device_only in (False, True):
        ctx = api.Context(s.scene)
        ctx.upload_seeds(s.seeds)
        ctx.set_pipelining(1, 0)
        capfd.readouterr()
        got = _call(ctx, s, sets, path, first_device_only)
        err = capfd.readouterr().err
        assert "staging area" in err and "needed" in err, err[-600:]
        _same(clouds[path], got, (path, "first call", first_device_only))
        again = _call(ctx, s, sets, path, not first_device_only)
        assert "staging area" not in capfd.readouterr().err
        _same(clouds[path], again, (path, "second call", not first_device_only))
        ctx.close()


@pytest.mark.parametrize("lanes,units", [(3, 5), (1, 0)])
def test_every_retry_of_stage_b_in_one_call(eg3d_form, monkeypatch, capfd, lanes, units):
    """All the knobs at once on a fresh context, the expand stage also cut into several launches (EG3D_MAX_SCRATCH_MB): K2
    runs again, the hypothesis arena is redone, chains that outgrew their slices are relaunched round after round, and
    the launch that finally fits its slices does not fit the staging area and is repeated whole — in one unit, and in
    five units on three lanes that each start from nothing. Host call and device-only call: byte-identical to the
    unforced, uncut call."""
    s, sets, clouds = _base(eg3d_form)
    for k, v in (("EG3D_HITS_CAP0", "1"), ("EG3D_ARENA_CAP0", "64"), ("EG3D_CHAIN_CAP0", "8"), ("EG3D_POOL_CAP0", "64"),
                 ("EG3D_STAGE_CAP0", "1"), ("EG3D_MAX_SCRATCH_MB", "4"), ("EG3D_TRACE_ARENA", "1")):
        monkeypatch.setenv(k, v)
    ctx = api.Context(s.scene)
    ctx.upload_seeds(s.seeds)
    ctx.set_pipelining(lanes, units)
    capfd.readouterr()
    got = _call(ctx, s, sets, "seeds", False)
    err = capfd.readouterr().err
    for msg in ("K2 runs again", "OVERFLOW", "relaunching those", "staging area"):
        assert msg in err, (msg, err[-800:])
    _same(clouds["seeds"], got, ("host", lanes, units))
    _same(clouds["seeds"], _call(ctx, s, sets, "seeds", True), ("device", lanes, units))
    ctx.close()
    # ... and a context whose FIRST call is the device-only one
    ctx = api.Context(s.scene)
    ctx.upload_seeds(s.seeds)
    ctx.set_pipelining(lanes, units)
    capfd.readouterr()
    got = _call(ctx, s, sets, "seeds", True)
    err = capfd.readouterr().err
    for msg in ("K2 runs again", "OVERFLOW", "relaunching those", "staging area"):
        assert msg in err, (msg, err[-800:])
    _same(clouds["seeds"], got, ("device first", lanes, units))
    ctx.close()
