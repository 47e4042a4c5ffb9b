"""-m gpu: the three builds of the expand kernel (k3b_expand small / many views / general, chosen per context by
launch_expand) on the scenes of tests/expand_boundary_cases.py, which stand on either side of the capacities the builds
are cut at — which scene is for which boundary, and which boundaries no scene reaches, is listed in
tests/test_expand_boundary_cases.py, where the CPU half shows that the reference run of every scene really reaches what
it is meant to reach.

Every scene runs match_refpoints and match_polyline_sets against the oracle (bit for bit: cloud, counts, flags,
algorithmic bytes), once per DLT form, under
  * the build launch_expand picks for the scene's class,
  * EG3D_K3B_FULL=1: the general build, which stands on both sides of tmp_cap <= 64 and of the vertex limit,
  * EG3D_K3B_ASSUME_SHORT=1 on v29, v31 and v33: the small build beyond its view count, where it must refuse a solve of
    more than 32 rows — exactly when the reach table says one is attempted — and the host redo the chunk with the
    general build.
The switches are read by eg3d_create, so every setting gets a fresh context. Expected verdicts come from the reach table
of the scene and form (computed on the CPU from the oracle and the host compilation of the stage), never from constants
here. The oracle's clouds are computed once per scene and form and shared, unchanged, by the tests of this module."""
import pytest

import expand_boundary_cases as ebc
from edgegraph3d_amd import api
from parity_util import compare_edgepoints

pytestmark = pytest.mark.gpu

REDONE = "a solve of more than 32 rows -> general build"
assert ebc.GN_PACK_MAX == 32, "the host's trace line names the capacity"


def _check(ref, got, what):
    rep = compare_edgepoints(ref, got)
    assert rep["ok"] and rep["bitexact_X"] and rep["bitexact_xy"], (what, rep["msgs"][:3])
    assert (got["flags"] & 7) == 0, (what, "device capacity flag raised", got["flags"])
    assert got["flags"] == ref["flags"], what
    assert got["n_chains"] == ref["stats"]["n_chains"] and got["n_tasks"] == ref["stats"]["n_tasks"], what
    assert got["times"]["bytes_algorithmic"] == ref["stats"]["bytes_algorithmic"], what
    assert got["n_points"] > 1000, what


def _run(name, rows, capfd, refusal_expected, calls=1):
    """A fresh context on the scene: `calls` x match_refpoints (the redo line must appear on the first call exactly when
    refusal_expected, and never again: the general build is latched), then match_polyline_sets."""
    c = ebc.case(name)
    ref, ref_sets = ebc.oracle_cloud(name, rows), ebc.oracle_cloud(name, rows, True)
    ctx = api.Context(c.scene)
    try:
        for call in range(calls):
            capfd.readouterr()
            got = ctx.match_refpoints(c.seeds)
            err = capfd.readouterr().err
            _check(ref, got, "%s match_refpoints, call %d" % (name, call))
            assert err.count(REDONE) == (1 if refusal_expected and call == 0 else 0), (name, call, refusal_expected, err[-400:])
        _check(ref_sets, ctx.match_polyline_sets(*c.sets), "%s match_polyline_sets" % name)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ebc.NAMES)
def test_the_build_of_the_scene_class(eg3d_form, monkeypatch, capfd, name):
    """The default build. Only the small build can refuse a solve; whether it must is the reach table's verdict (on v28,
    with points of 29 observations, it must not)."""
    monkeypatch.delenv("EG3D_K3B_FULL", raising=False)
    monkeypatch.delenv("EG3D_K3B_ASSUME_SHORT", raising=False)
    monkeypatch.setenv("EG3D_TRACE_ARENA", "1")
    t = ebc.reach_table(name, eg3d_form)
    _run(name, eg3d_form, capfd, t["scene_class"] == "small" and ebc.long_solve_expected(t))


@pytest.mark.parametrize("name", ebc.NAMES)
def test_the_general_build(eg3d_form, monkeypatch, capfd, name):
    monkeypatch.delenv("EG3D_K3B_ASSUME_SHORT", raising=False)
    monkeypatch.setenv("EG3D_K3B_FULL", "1")
    monkeypatch.setenv("EG3D_TRACE_ARENA", "1")
    _run(name, eg3d_form, capfd, False)


@pytest.mark.parametrize("name", ["v29", "v31", "v33"])
def test_the_small_build_beyond_its_view_count_refuses_exactly_the_solves_it_cannot_pack(eg3d_form, monkeypatch, capfd, name):
    """EG3D_K3B_ASSUME_SHORT=1: the small build at 29, 31 and 33 views (its N-view step lists in the chain's slice).
    v31's largest solve is exactly 32 rows — the fullest packed round, nothing refused; v33 attempts 33 and 34 rows —
    refused once, the chunk redone by the general build, which stays latched for the second call."""
    monkeypatch.delenv("EG3D_K3B_FULL", raising=False)
    monkeypatch.setenv("EG3D_K3B_ASSUME_SHORT", "1")
    monkeypatch.setenv("EG3D_TRACE_ARENA", "1")
    t = ebc.reach_table(name, eg3d_form)
    assert ebc.case(name).scene_class == "many views"   # (otherwise the switch would not pick the small build)
    _run(name, eg3d_form, capfd, ebc.long_solve_expected(t), calls=2)
