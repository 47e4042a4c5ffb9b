"""-m gpu: the single-pass K2 (k2_epipolar_hits, eg3d_k1_k2_refpoints.hip). One wavefront per task stages the task's epipolar hits
in LDS, claims its region of the hit buffer with one atomicAdd and copies the stage out; a task with more hits than the
stage holds (EG3D_K2_STAGE_CAP, default 128) takes the count - claim - write route instead; a hit buffer that turns out
too small (EG3D_HITS_CAP0 forces it) is enlarged by the host and K2 runs again. Where a task's hits lie in the buffer
depends on timing, so everything here compares what is addressed THROUGH the lists — the stage-A arrays of
Context.candidates, which gathers in (task, list) order, and whole clouds — with the CPU oracle, bit for bit."""
import ctypes as C
import threading

import numpy as np
import pytest

from edgegraph3d_amd import api, host
from parity_util import compare_edgepoints

pytestmark = pytest.mark.gpu

ARRAYS = ("X", "obs_off", "obs_view", "obs_pl", "obs_seg", "obs_xy", "key")
DEFAULT_STAGE_CAP = 128   # EG3D_K2_STAGE_MAX of eg3d_kernels.h


def _oracle(scene):
    from oracle import binding as ob
    return ob.Oracle(scene)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_stage_a(got, ref, what):
    for k in ref:
        x, y = got[k], ref[k]
        if isinstance(y, np.ndarray):
            assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, k)
        else:
            assert x == y, (what, k, x, y)


def _same_cloud(a, b, what):
    for k in ("n_points", "n_obs", "n_tasks", "n_hypotheses", "n_chains", "flags"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ARRAYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)


_REF = {}


def _ref(cfg):
    """Oracle results of host.Synth(cfg), computed once and shared (read-only)."""
    if cfg not in _REF:
        s = host.Synth(cfg)
        o = _oracle(s.scene)
        _REF[cfg] = (s, o.candidates(s.seeds, 0, s.n_seeds), o.match(s.seeds, 0, s.n_seeds, nthreads=8))
    return _REF[cfg]


def _hits_per_task(cand):
    lo, tl = cand["list_off"], cand["task_list_off"]
    return lo[tl[1:]].astype(np.int64) - lo[tl[:-1]].astype(np.int64)


@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("stage_cap", ["1", "4", None], ids=["cap1", "cap4", "default"])
def test_stage_a_and_cloud_equal_the_oracle_whatever_the_stage_holds(monkeypatch, cfg, stage_cap):
    """A stage of one hit sends every task with more than its start hit down the unstaged route (3/4 of the tasks of
    these scenes), a stage of 4 those with more than 4 (none of Synth(0), whose tasks have at most 4 hits, a fifth of
    Synth(1)'s), the default none: the same arrays and the same cloud."""
    s, ref_cand, ref_cloud = _ref(cfg)
    per_task = _hits_per_task(ref_cand)
    assert (per_task > 1).mean() > 0.5 and per_task.max() <= DEFAULT_STAGE_CAP
    assert cfg == 0 or (per_task > 4).any()
    if stage_cap is not None:
        monkeypatch.setenv("EG3D_K2_STAGE_CAP", stage_cap)
    ctx = api.Context(s.scene)
    _same_stage_a(ctx.candidates(s.seeds, 0, s.n_seeds), ref_cand, stage_cap)
    got = ctx.match_refpoints(s.seeds)
    ctx.close()
    rep = compare_edgepoints(ref_cloud, got)
    assert rep["ok"] and rep["bitexact_X"] and rep["bitexact_xy"], rep["msgs"][:3]
    assert got["n_tasks"] == ref_cloud["stats"]["n_tasks"] and got["n_chains"] == ref_cloud["stats"]["n_chains"]


@pytest.mark.parametrize("cfg", [0, 1])
def test_a_hit_buffer_that_is_too_small_is_enlarged_and_k2_runs_again(monkeypatch, capfd, cfg):
    """EG3D_HITS_CAP0=1: the first K2 launch of the context has room for one hit, every task's claim ends beyond it. The
    host sees the cursor in its next read-back, enlarges the buffer and launches K2 again (the trace says so): same
    arrays, same cloud. What the context has learned then serves the next call without a second launch."""
    s, ref_cand, ref_cloud = _ref(cfg)
    monkeypatch.setenv("EG3D_HITS_CAP0", "1")
    monkeypatch.setenv("EG3D_TRACE_ARENA", "1")
    ctx = api.Context(s.scene)
    ctx.set_pipelining(1, 0)
    capfd.readouterr()
    got = ctx.match_refpoints(s.seeds)
    assert capfd.readouterr().err.count("K2 runs again") == 1
    rep = compare_edgepoints(ref_cloud, got)
    assert rep["ok"] and rep["bitexact_X"] and rep["bitexact_xy"], rep["msgs"][:3]
    again = ctx.match_refpoints(s.seeds)
    assert "K2 runs again" not in capfd.readouterr().err
    _same_cloud(got, again, "second call")
    _same_stage_a(ctx.candidates(s.seeds, 0, s.n_seeds), ref_cand, "after the retry")
    ctx.close()
    # the debug export has the same retry of its own
    ctx = api.Context(s.scene)
    capfd.readouterr()
    _same_stage_a(ctx.candidates(s.seeds, 0, s.n_seeds), ref_cand, "retry inside candidates")
    assert capfd.readouterr().err.count("K2 runs again") == 1
    ctx.close()


def _hand_made_scene():
    """host.Synth(0) with, around every observation of seed 0, a comb of 120 long parallel 2-vertex polylines 4 .. 10 px
    from the observation (each one a candidate AND a start hit, so the seed gets ~120 tasks per entry whose detection
    radius of 12 .. 30 px takes in most of the other views' combs: > 64 candidates per list, > 128 hits per task). One
    tooth of each comb is cut into 320 collinear segments. The fundamental matrices of one view outside seed 0's track
    are invalid: lists towards it are empty, and a task that starts in it has nothing but its start hit."""
    s = host.Synth(0)
    sc = s.scene_np()
    off, view, xy = s.seeds_np()
    V = int(sc["n_views"])
    vpo, pvo, vtx = sc["view_pl_off"], sc["pl_vtx_off"], sc["vtx_xy"]
    node0 = int(max(sc["pl_start"].max(), sc["pl_end"].max())) + 1
    n_vpo, n_pvo, n_vtx, n_st, n_en, n_val = [0], [0], [], [], [], []
    for v in range(V):
        for g in range(int(vpo[v]), int(vpo[v + 1])):   # the view's own polylines, unchanged
            n_vtx.extend(vtx[pvo[g]:pvo[g + 1]])
            n_pvo.append(len(n_vtx))
            n_st.append(sc["pl_start"][g]); n_en.append(sc["pl_end"][g]); n_val.append(sc["pl_valid"][g])
        for e in range(int(off[0]), int(off[1])):
            if view[e] != v:
                continue
            ang = 0.4 + 0.9 * v
            d = np.array([np.cos(ang), np.sin(ang)])      # along the teeth
            n = np.array([-d[1], d[0]])                   # across them
            for i in range(120):
                mid = xy[e].astype(np.float64) + n * (4.0 + 0.05 * i)
                a, b = mid - 40.0 * d, mid + 40.0 * d
                pieces = 320 if i == 7 else 1
                pts = [(a + (b - a) * (j / pieces)).astype(np.float32) for j in range(pieces + 1)]
                n_vtx.extend(pts)
                n_pvo.append(len(n_vtx))
                n_st.append(node0); n_en.append(node0 + 1); n_val.append(1)
                node0 += 2
        n_vpo.append(len(n_pvo) - 1)
    sc["view_pl_off"] = np.asarray(n_vpo, np.uint32)
    sc["pl_vtx_off"] = np.asarray(n_pvo, np.uint32)
    sc["vtx_xy"] = np.asarray(n_vtx, np.float32).reshape(-1, 2)
    sc["pl_start"], sc["pl_end"] = np.asarray(n_st, np.uint32), np.asarray(n_en, np.uint32)
    sc["pl_valid"] = np.asarray(n_val, np.uint8)
    dead = [v for v in range(V) if v not in set(int(x) for x in view[off[0]:off[1]])][0]
    Fv = sc["F_valid"].copy()
    Fv[dead, :] = 0
    Fv[:, dead] = 0
    sc["F_valid"] = Fv
    return s, sc, host.SceneArrays(sc)


def test_hand_made_lists_empty_crowded_long_and_larger_than_the_stage(monkeypatch):
    """Stage A on a scene built for K2's paths, at the default stage and with a stage of 1. The oracle's arrays say which
    cases the scene holds; each is asserted before the comparison: an empty list, the start-view list (every task has
    one: its single hit is the start hit), a list fed by >= 65 candidate polylines, a candidate polyline of >= 300
    segments (more than one trip of 4 x 64 flat segments), a task all of whose epipolar lists are empty (only the
    start-view list holds its one hit), and a task with more hits than the default stage."""
    s, sc, sa = _hand_made_scene()
    n = 8   # seed 0 (the combs) and a few ordinary seeds
    ref = _oracle(C.byref(sa.c)).candidates(s.seeds, 0, n)
    per_list = np.diff(ref["list_off"])
    per_task = _hits_per_task(ref)
    per_entry = np.diff(ref["cand_off"])
    assert (per_list == 0).any(), "no empty list"
    assert per_task.min() == 1, "no task whose epipolar lists are all empty"
    assert (per_task >= 1).all()   # the start-view list is never empty
    assert per_entry.max() >= 65, per_entry.max()
    assert per_task.max() > DEFAULT_STAGE_CAP, per_task.max()
    segs = np.diff(sc["pl_vtx_off"]) - 1
    off, view, _ = s.seeds_np()
    long_is_candidate = False
    for sv in range(len(per_entry)):
        v = int(view[sv])
        ids = ref["cand_pl"][ref["cand_off"][sv]:ref["cand_off"][sv + 1]]
        if len(ids) and segs[int(sc["view_pl_off"][v]) + ids].max() >= 300:
            long_is_candidate = True
    assert long_is_candidate, "no candidate polyline of >= 300 segments"
    for cap in (None, "1"):
        if cap is not None:
            monkeypatch.setenv("EG3D_K2_STAGE_CAP", cap)
        ctx = api.Context(C.byref(sa.c))
        _same_stage_a(ctx.candidates(s.seeds, 0, n), ref, cap)
        ctx.close()


def test_two_clones_driven_from_two_threads_give_the_serial_clouds():
    """The cursor the tasks claim from belongs to the context: two clones that run their steps at the same time (two
    host threads, the way bench.py keeps steps in flight) produce the clouds one context produces serially."""
    s, _, ref_cloud = _ref(1)
    n = s.n_seeds
    ranges = [(0, n // 2), (n // 2, n)]
    ctx = api.Context(s.scene)
    ctx.upload_seeds(s.seeds)
    ctx.set_pipelining(1, 0)
    serial = [ctx.match_resident(b, e) for b, e in ranges]
    whole = ctx.match_resident(0, n)
    rep = compare_edgepoints(ref_cloud, whole)
    assert rep["ok"] and rep["bitexact_X"] and rep["bitexact_xy"], rep["msgs"][:3]
    clones = [ctx.clone(), ctx.clone()]
    for c in clones:
        c.set_pipelining(1, 0)
    out, errs = [[None] * 4, [None] * 4], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            gate.wait()
            for r in range(4):   # both ranges on both clones, in opposite orders, twice
                b, e = ranges[(i + r) % 2]
                out[i][r] = ((i + r) % 2, clones[i].match_resident(b, e))
        except Exception as ex:   # noqa: BLE001 (reported below)
            errs.append(ex)
            gate.abort()

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        for which, got in out[i]:
            _same_cloud(serial[which], got, ("clone", i, which))
    for c in clones:
        c.close()
    ctx.close()
