"""CPU half of the expand kernel's boundary scenes (tests/expand_boundary_cases.py): for every named scene, in both forms
of the DLT system,

  * the host compilation of the stage (tests/hostsim: eg3d_dev_expand.h with the one-member team) equals the oracle bit
    for bit with no capacity flag — on the run whose side walks, solves and N-view steps the reach table counts;
  * the REACH CONDITIONS hold: the reference run of the scene really stands where the scene is meant to stand. They
    are conditions on the scenes, computed from the oracle and the host compilation alone; a scene that misses one
    gets another seed or size, the condition stays.

Which boundary each scene is for (capacities: expand_boundary_cases.py):

  v28          the last view count of the small build: V = 28, tmp_cap = 64 = COOP_ROWS (the N-view step's list in LDS,
               the look-ahead rounds on); points of 28 and of 29 observations (a view repeated), solves of up to 29
               rows and no refusal; side walks past the 96 staged lines
  v29          the first view count of the many-views build, and of the list in the chain's slice (tmp_cap = 66), in
               the many-views and the general build; under EG3D_K3B_ASSUME_SHORT the small build with its list in the
               slice; side walks past the 96 staged lines
  v27          one below: side walks past the 96 staged lines on BOTH sides of an attachment (a chain of >= 194 points)
  v31          the fullest packed round: the largest solve attempted is exactly GN_PACK_MAX = 32 rows, so the small
               build (EG3D_K3B_ASSUME_SHORT) must solve everything and refuse nothing
  v33          solves of 33 and 34 rows: the small build must refuse, the host latch the general build and redo
  vtx512       the longest valid polyline is exactly STAGE_VTX = 512 vertices: the staging area exactly full (small)
  vtx513       valid polylines of 513 and of 512 vertices side by side: the general build's unstaged and staged walks
  v29_vtx512   the many-views build at its vertex limit
  v29_vtx513   the general build at V >= 29 with both walk routes
  v27 v28      N-view steps whose later starting observations start from lists of n <= 21 and of 22 <= n <= 28:
               stepn_walks_par with 64 / n >= 3 and = 2 candidates per pass

LEFT UNTESTED, because no scene of this size reaches it (or none can):
  * stepn_walks_par with 64 / n < 2 (n >= 33), its sequential fall-back. It is only called from the look-ahead rounds,
    which run when the list is in LDS (V <= 28) and two lists fit it (n <= 32); lists of 32 and of 33 exist in v33 (the
    conditions below show them), but there the following goes one step at a time. As the callers stand the branch cannot
    be reached.
  * two look-ahead lists that fill CoopLds::tmp_a to the last row (n = 32 at V <= 28): the longest list of v28 is 28.
  * a side walk of more than 96 lines on a polyline of 512 / 513 vertices: the vertex scenes at 6 views walk at most
    53 lines, the 29-view ones do exceed 96 lines (v29_vtx512, v29_vtx513: see their tables).
  * an INVALID polyline longer than 512 vertices in a scene whose valid ones all fit (the host's rule counts the valid
    ones only): the invalid polylines of the synthetic scenes are empty."""
import numpy as np
import pytest

import expand_boundary_cases as ebc
import forms
from parity_util import compare_edgepoints


def _some(hist, lo, hi=None):
    return any(lo <= n and (hi is None or n <= hi) for n in hist)


def reach_conditions(t):
    """[(condition, holds)] of the scene of table t."""
    name, h = t["name"], t["obs_histogram"]
    c = []
    if name == "v28":
        c += [("V == 28", t["n_views"] == 28), ("no valid polyline above 512 vertices", t["longest_valid_polyline"] <= ebc.STAGE_VTX),
              ("a point of 28 observations", h.get(28, 0) >= 1), ("a point of 29 observations", h.get(29, 0) >= 1),
              ("largest solve attempted <= 32 rows", t["solve_rows_max"] <= ebc.GN_PACK_MAX),
              ("longest side walk > 96", t["side_walk_max"] > ebc.EPI_HALF), ("small build", t["scene_class"] == "small")]
    if name == "v29":
        c += [("V == 29", t["n_views"] == 29), ("a point of >= 29 observations", _some(h, 29)),
              ("longest side walk > 96", t["side_walk_max"] > ebc.EPI_HALF), ("many-views build", t["scene_class"] == "many views")]
    if name == "v27":
        c += [("V == 27", t["n_views"] == 27), ("longest side walk > 96", t["side_walk_max"] > ebc.EPI_HALF),
              ("a chain of >= 194 points", t["longest_chain"] >= 2 * ebc.EPI_HALF + 2), ("small build", t["scene_class"] == "small")]
    if name == "v31":
        c += [("largest solve attempted == 32 rows", t["solve_rows_max"] == ebc.GN_PACK_MAX), ("V >= 29", t["n_views"] >= 29)]
    if name == "v33":
        c += [("largest solve attempted >= 33 rows", t["solve_rows_max"] >= ebc.GN_PACK_MAX + 1)]
    if name.endswith("vtx512"):
        c += [("longest valid polyline == 512", t["longest_valid_polyline"] == ebc.STAGE_VTX),
              ("more than 1000 points", t["n_points"] > 1000),
              ("observations on polylines of 512 vertices", t["obs_on_polylines_at_most_stage_vtx"] > 0)]
    if name.endswith("vtx513"):
        c += [("longest valid polyline == 513", t["longest_valid_polyline"] == ebc.STAGE_VTX + 1),
              ("a valid polyline of <= 512 vertices", t["valid_polylines_at_most_stage_vtx"] >= 1),
              ("... that carries observations of the cloud", t["obs_on_polylines_at_most_stage_vtx"] > 0),
              ("observations on polylines of 513 vertices", t["obs_on_polylines_longer"] > 0),
              ("more than 1000 points", t["n_points"] > 1000), ("general build", t["scene_class"] == "general")]
    if name.startswith("v29_"):
        c += [("V == 29", t["n_views"] == 29), ("longest side walk > 96", t["side_walk_max"] > ebc.EPI_HALF)]
    if name == "v29_vtx512":
        c += [("many-views build", t["scene_class"] == "many views")]
    if name == "vtx512":
        c += [("small build", t["scene_class"] == "small")]
    assert c, name
    return c


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
@pytest.mark.parametrize("name", ebc.NAMES)
def test_scene_reaches_its_boundary_and_the_host_compilation_equals_the_oracle(name, rows):
    ref = ebc.oracle_cloud(name, rows)
    sim, _ = ebc.hostsim_run(name, rows)
    rep = compare_edgepoints(ref, sim)
    assert rep["ok"] and rep["bitexact_X"] and rep["bitexact_xy"], rep["msgs"][:3]
    assert (sim["flags"] & 7) == 0, "a capacity of the host simulation overflowed: %d" % sim["flags"]
    assert sim["flags"] == ref["flags"]
    assert sim["n_chains"] == ref["stats"]["n_chains"] and sim["n_tasks"] == ref["stats"]["n_tasks"]
    t = ebc.reach_table(name, rows)
    print("\n" + ebc.describe(t))
    missed = [text for text, holds in reach_conditions(t) if not holds]
    assert not missed, (missed, ebc.describe(t))


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_the_scenes_together_stand_on_both_sides_of_the_candidates_per_pass_rule(rows):
    """stepn_walks_par packs 64 / n starting observations to a pass and falls back to one at a time when that is < 2:
    lists of n == 32 and of n >= 33 exist (the two sides of the rule), and lists of 22..32 and of <= 21 (2 and >= 3 per
    pass) — among the lists a LATER starting observation is walked from, which is when the kernel packs, at view counts
    where it does (the list in LDS: V <= 28) for the last two."""
    tables = [ebc.reach_table(n, rows) for n in ebc.NAMES]
    every = [set(t["step_first"]) | set(t["step_later"]) for t in tables]
    assert any(32 in h for h in every), "no N-view step list of 32"
    assert any(_some(h, 33) for h in every), "no N-view step list of >= 33"
    assert any(_some(h, 22, 32) for h in every) and any(_some(h, 1, 21) for h in every)
    packed = [t["step_later"] for t in tables if t["n_views"] <= ebc.SMALL_VIEWS]
    assert any(_some(h, 22, 32) for h in packed), "no later candidate at 2 per pass where the kernel packs them"
    assert any(_some(h, 3, 21) for h in packed), "no later candidate at >= 3 per pass where the kernel packs them"
    # the refusal rule has a scene on either side of it, and one exactly on it
    rows_max = {t["name"]: t["solve_rows_max"] for t in tables}
    assert rows_max["v31"] == ebc.GN_PACK_MAX < rows_max["v33"] and rows_max["v28"] < ebc.GN_PACK_MAX, rows_max


def test_resampling_keeps_every_vertex_and_hits_the_vertex_counts_exactly():
    """The resampled polylines are the original ones with collinear vertices added: every original vertex is still
    there, in order, the ends are unchanged, and the valid polylines of >= 20 vertices have exactly 512 (vtx512) or
    alternately 513 and 512 (vtx513) vertices; shorter ones are untouched."""
    from edgegraph3d_amd import host
    base = host.Synth(1).scene_np()
    n0 = np.diff(base["pl_vtx_off"].astype(np.int64))
    for longest in (512, 513):
        sc = ebc.resample(base, longest)
        n1 = np.diff(sc["pl_vtx_off"].astype(np.int64))
        big = (n0 >= ebc.RESAMPLE_MIN) & (base["pl_valid"] != 0)
        assert big.sum() > 50 and np.array_equal(n1[~big], n0[~big])
        want = np.full(int(big.sum()), longest)
        if longest > ebc.STAGE_VTX:
            want[1::2] = ebc.STAGE_VTX
        assert np.array_equal(n1[big], want)
        for p in np.nonzero(big)[0][:12]:
            a = base["vtx_xy"][base["pl_vtx_off"][p]:base["pl_vtx_off"][p + 1]]
            b = sc["vtx_xy"][sc["pl_vtx_off"][p]:sc["pl_vtx_off"][p + 1]]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[-1], b[-1])
            k = 0
            for v in b:                     # a is a subsequence of b
                if k < len(a) and np.array_equal(v, a[k]):
                    k += 1
            assert k == len(a), (p, k, len(a))
        for key in ("pl_start", "pl_end", "pl_valid", "view_pl_off", "cam_P", "F"):
            assert np.array_equal(sc[key], base[key])
