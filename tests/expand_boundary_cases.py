"""Scenes that stand on either side of the capacities the three builds of the expand kernel (k3b_expand: small, many
views, general — launch_expand in edgegraph3d_amd/csrc/eg3d_api_match_stage_b.hip) are cut at, and, per scene, the REACH TABLE:
what the reference run of the scene reaches, computed on the CPU. Shared by the CPU half
(tests/test_expand_boundary_cases.py: the reach conditions, and the host compilation of the stage against the oracle)
and the GPU half (tests/test_gpu_expand_boundaries.py: the three builds against the oracle, the expected verdicts
taken from the table).

The capacities (read from the headers' text below, so a changed capacity moves the conditions with it):

  COOP_ROWS = 64      tmp_cap = 2 V + 8 <= 64 (V <= 28): the N-view step's candidate list lives in CoopLds::tmp_a, and the
                      chain following walks ahead; V >= 29: the list lives in the chain's slice, one step at a time
  GN_PACK_MAX = 32    a solve of more rows needs the solver's long-request path, which the small build lacks: it raises
                      CTR_LONG_REFUSED and the host redoes the chunk with the general build
  STAGE_VTX = 512     the side walks stage a polyline of at most this many vertices in LDS; only the general build walks
                      a longer one
  STAGE_EPI / 2 = 96  epipolar lines staged per side of a side walk; the 97th line and later are read from Chain::cand
  64 / n              starting observations per pass of stepn_walks_par (n = length of the list the step starts from)

The scenes:

  v27 v28 v29 v31 v33           host.default_config(1) with rng_seed = 13 + V, n_views = V, n_curves = 24, max_track = V,
                                n_seeds = 80 (the recipe of test_scene_class_builds_of_the_expand_kernel_agree_with_the_
                                general_one)
  vtx512 vtx513                 Synth(1) with the segments of every polyline of >= RESAMPLE_MIN vertices split evenly into
                                collinear pieces: the valid ones to exactly 512 vertices (vtx512), or alternately to 513
                                and 512 (vtx513: staged and unstaged walks at the limit in one scene); the shorter
                                polylines stay as they are (the invalid polylines of these scenes are empty)
  v29_vtx512 v29_vtx513         the same resampling of v29

Reach table of a scene and a DLT form (reach_table): the view count, the longest valid polyline, the histogram of
observations per point and the longest chain of the ORACLE's cloud, and three counts the cloud cannot tell (rejected
attempts leave no trace in it), taken from the host compilation of eg3d_dev_expand.h (tests/hostsim, EG3D_REACH), which
the CPU half shows to equal the oracle bit for bit on the very run that is counted:
  side_walk_max    most epipolar lines one side walk (walk_side_candidates_core) consumed: > 96 means a walk went on
                   with the line of slot 96, the first one that is not staged
  solve_rows_max   rows of the largest solve attempted, the extra row of an ADD request included
  step_first / step_later   {n: events}: length n of the list an N-view step's first / a later starting observation
                   was walked from (a later one is what stepn_walks_par packs 64 / n to a pass)
Nothing in the table comes from the code under test on the GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np

import forms
import hostsim_binding as hs
from edgegraph3d_amd import host
from parity_util import chain_ranges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(header, name):
    text = open(os.path.join(ROOT, "edgegraph3d_amd", "csrc", header)).read()
    m = re.search(r"#define\s+%s\s+([0-9]+)\b" % name, text)
    assert m, (header, name)
    return int(m.group(1))


COOP_ROWS = _header_constant("eg3d_dev_coopgn.h", "EG3D_COOP_ROWS")
GN_PACK_MAX = _header_constant("eg3d_dev_coopgn.h", "EG3D_GN_PACK_MAX")
STAGE_VTX = _header_constant("eg3d_dev_coopgn.h", "EG3D_STAGE_VTX")
EPI_HALF = _header_constant("eg3d_dev_coopgn.h", "EG3D_STAGE_EPI") // 2
SMALL_VIEWS = _header_constant("eg3d_kernels.h", "EG3D_SMALL_SCENE_VIEWS_HOST")
assert (COOP_ROWS, GN_PACK_MAX, STAGE_VTX, EPI_HALF, SMALL_VIEWS) == (64, 32, 512, 96, 28), \
    "a capacity of the expand kernel changed: the named scenes below were chosen for 64 / 32 / 512 / 96 / 28"

VIEW_SCENES = {"v27": 27, "v28": 28, "v29": 29, "v31": 31, "v33": 33}
NAMES = tuple(VIEW_SCENES) + ("vtx512", "vtx513", "v29_vtx512", "v29_vtx513")
RESAMPLE_MIN = 20      # polylines of at least this many vertices are resampled
# capacities of the host simulation (hypothesis points, chain points, observation pool): its defaults overflow on the
# scenes of 27 and 28 views
HOSTSIM_CAPS = dict(hyp_cap=400, chain_cap=2048, pool_cap=65536)
ORACLE_THREADS = 16
N_SETS = 3


def recipe(n_views):
    cfg = host.default_config(1)
    cfg.rng_seed, cfg.n_views, cfg.n_curves, cfg.max_track, cfg.n_seeds = 13 + n_views, n_views, 24, n_views, 80
    return cfg


def resample(sc, longest):
    """The scene arrays `sc` (Synth.scene_np) with every valid polyline of >= RESAMPLE_MIN vertices resampled: the j-th one to
    `longest` vertices if longest <= STAGE_VTX, else alternately to `longest` and STAGE_VTX. A polyline of n vertices goes to
    T by cutting each of its n - 1 segments into (T - 1) // (n - 1) pieces, the first (T - 1) % (n - 1) segments into one
    more; the new vertices are v[i] + (v[i + 1] - v[i]) * (k / K) in FP32."""
    pvo, vtx, valid = sc["pl_vtx_off"], sc["vtx_xy"], sc["pl_valid"]
    new_off, new_vtx, j = [0], [], 0
    for p in range(len(pvo) - 1):
        v = vtx[pvo[p]:pvo[p + 1]]
        n = len(v)
        if n < RESAMPLE_MIN or not valid[p]:
            new_vtx.extend(v)
        else:
            T = longest if (longest <= STAGE_VTX or j % 2 == 0) else STAGE_VTX
            j += 1
            q, r = divmod(T - 1, n - 1)
            assert q >= 1, (n, T)
            for i in range(n - 1):
                K = q + (1 if i < r else 0)
                t = (np.arange(K, dtype=np.float32) / np.float32(K))[:, None]
                new_vtx.extend(v[i] + (v[i + 1] - v[i]) * t)
            new_vtx.append(v[-1])
            assert len(new_vtx) - new_off[-1] == T
        new_off.append(len(new_vtx))
    out = dict(sc)
    out["pl_vtx_off"] = np.asarray(new_off, np.uint32)
    out["vtx_xy"] = np.asarray(new_vtx, np.float32).reshape(-1, 2)
    return out


class Case:
    """One named scene: .scene / .seeds (ctypes pointers for api.Context, the oracle and the host simulation), .n_seeds,
    .sets = (n_sets, row_off, ids) of Synth.polyline_sets(N_SETS), .arrays (Synth.scene_np of what .scene points to)."""

    def __init__(self, name):
        assert name in NAMES, name
        self.name = name
        base, _, vtx = name.rpartition("_") if "vtx" in name else (name, "", "")
        self.synth = host.Synth(recipe(VIEW_SCENES[base])) if base else host.Synth(1)
        self.seeds, self.n_seeds = self.synth.seeds, self.synth.n_seeds
        self.sets = self.synth.polyline_sets(N_SETS)
        if vtx:
            self.arrays = resample(self.synth.scene_np(), int(vtx[3:]))
            self._owner = host.SceneArrays(self.arrays)
            self.scene = C.pointer(self._owner.c)
        else:
            self.arrays = self.synth.scene_np()
            self.scene = self.synth.scene

    @property
    def n_views(self):
        return int(self.arrays["n_views"])

    def valid_polyline_sizes(self):
        return np.diff(self.arrays["pl_vtx_off"].astype(np.int64))[self.arrays["pl_valid"] != 0]

    @property
    def scene_class(self):
        """The build launch_expand picks for the scene by default: 'small', 'many views' or 'general'."""
        if int(self.valid_polyline_sizes().max()) > STAGE_VTX:
            return "general"
        return "many views" if self.n_views > SMALL_VIEWS else "small"


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def oracle_cloud(name, rows, sets=False):
    """The oracle's cloud of match_refpoints (sets: of match_polyline_sets on the case's sets) in the DLT form `rows`:
    computed once per process, never changed by the tests that share it."""
    from oracle import binding as ob
    c = case(name)
    with forms.oracle_rows(rows):
        o = ob.Oracle(c.scene)
        r = o.match_polyline_sets(*c.sets, nthreads=ORACLE_THREADS) if sets else o.match(c.seeds, 0, c.n_seeds, nthreads=ORACLE_THREADS)
        o.close()
    return r


@functools.lru_cache(maxsize=None)
def hostsim_run(name, rows):
    """(cloud of the host compilation of the stage from the oracle's stage-A candidates, its reach histograms)."""
    from oracle import binding as ob
    c = case(name)
    with forms.oracle_rows(rows):
        o = ob.Oracle(c.scene)
        cand = o.candidates_raw(c.seeds, 0, c.n_seeds)
        sim = hs.match(c.scene, c.seeds, 0, c.n_seeds, cand, rows=rows, **HOSTSIM_CAPS)
        hist = [hs.reach(k, rows=rows) for k in (hs.REACH_SIDE_WALK, hs.REACH_SOLVE_ROWS, hs.REACH_STEP_FIRST, hs.REACH_STEP_LATER)]
        ob.lib().orc_free_candidates(C.byref(cand))
        o.close()
    return sim, hist


@functools.lru_cache(maxsize=None)
def reach_table(name, rows):
    c = case(name)
    ref = oracle_cloud(name, rows)
    _, (walk, solve, first, later) = hostsim_run(name, rows)
    nobs = np.diff(ref["obs_off"].astype(np.int64))
    sizes = c.valid_polyline_sizes()
    short = sizes <= STAGE_VTX
    # observations of the cloud on valid polylines of at most STAGE_VTX vertices (global polyline id = view's first + local id)
    gid = c.arrays["view_pl_off"].astype(np.int64)[ref["obs_view"]] + ref["obs_pl"].astype(np.int64)
    pl_sizes = np.diff(c.arrays["pl_vtx_off"].astype(np.int64))
    return {
        "name": name, "dlt_rows": rows, "n_views": c.n_views, "scene_class": c.scene_class,
        "longest_valid_polyline": int(sizes.max()),
        "valid_polylines_at_most_stage_vtx": int(short.sum()), "valid_polylines_longer": int((~short).sum()),
        "obs_on_polylines_at_most_stage_vtx": int((pl_sizes[gid] <= STAGE_VTX).sum()),
        "obs_on_polylines_longer": int((pl_sizes[gid] > STAGE_VTX).sum()),
        "n_points": int(ref["n_points"]),
        "obs_histogram": {int(k): int(n) for k, n in enumerate(np.bincount(nobs)) if n},
        "longest_chain": max((b - a for a, b in chain_ranges(ref).values()), default=0),
        "side_walk_max": max(walk, default=0), "solve_rows_max": max(solve, default=0),
        "step_first": first, "step_later": later,
        "step_list_max": max(list(first) + list(later), default=0),
    }


def long_solve_expected(table):
    """Does a build without the solver's long-request path meet a solve it must refuse on this scene?"""
    return table["solve_rows_max"] > GN_PACK_MAX


def describe(table):
    t = table
    top = sorted(t["obs_histogram"])[-3:]
    return ("%-11s %s V=%d class=%s longest valid polyline %d, %d points, chain <= %d, observations per point <= %d "
            "(%s), side walk <= %d lines, solve <= %d rows, N-view step lists: first candidate n <= %d, later candidates n in %s"
            % (t["name"], forms.IDS[t["dlt_rows"]], t["n_views"], t["scene_class"], t["longest_valid_polyline"],
               t["n_points"], t["longest_chain"], top[-1],
               ", ".join("%d: %d" % (k, t["obs_histogram"][k]) for k in top), t["side_walk_max"], t["solve_rows_max"],
               max(t["step_first"], default=0), _ranges(sorted(t["step_later"]))))


def _ranges(v):
    out, i = [], 0
    while i < len(v):
        j = i
        while j + 1 < len(v) and v[j + 1] == v[j] + 1:
            j += 1
        out.append("%d" % v[i] if i == j else "%d..%d" % (v[i], v[j]))
        i = j + 1
    return "{" + ", ".join(out) + "}"
