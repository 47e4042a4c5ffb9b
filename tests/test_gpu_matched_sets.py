"""-m gpu: the pipelines 1-2 extractor when the caller's PLGMatchesManager holds intervals
(eg3d_match_polyline_sets_matched, eg3d_polyline_set_candidates: k_n1_samples / k_n1_hits <., true>, k_n1_check_intervals).

Stage A is compared exactly with the independent restatement tests/matched_ref.py (sample order, ids, coordinate bit
patterns, every hit list, both counts), with the intervals as host arrays and as the device arrays of eg3d_replay_device.
No reference can be fed explicit hit lists and stage B is untouched, so the end-to-end checks are identities against the
unfiltered call on the same sets. Tiny scenes throughout."""
import ctypes as C

import numpy as np
import pytest

import cbuild
import matched_ref as R
import sets_cases as cases
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host

pytestmark = pytest.mark.gpu

ARRAYS = ("X", "obs_off", "obs_view", "obs_pl", "obs_seg", "obs_xy", "key")
COUNTS = ("n_points", "n_obs", "n_tasks", "n_hypotheses", "n_chains", "flags")


def _ob():
    from oracle import binding as ob
    return ob


def _live():
    f = api.lib().eg3d_test_live_device_bytes
    f.restype, f.argtypes = C.c_int64, []
    return int(f())


def _same(a, b, what, skip=()):
    for k in COUNTS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ARRAYS:
        if k in skip:
            continue
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)


def _empty_graph(n_pl):
    return {"n_scene_polylines": n_pl, "iv_off": np.zeros(n_pl + 1, np.uint64), "iv_start_seg": np.zeros(0, np.uint32),
            "iv_start_xy": np.zeros((0, 2), np.float32), "iv_end_seg": np.zeros(0, np.uint32),
            "iv_end_xy": np.zeros((0, 2), np.float32)}


def _chains(cloud):
    """{sample (key[0]): bytes of everything its points carry but key[0]}"""
    out = {}
    key, off = cloud["key"], cloud["obs_off"].astype(np.int64)
    for p in range(cloud["n_points"]):
        a, b = int(off[p]), int(off[p + 1])
        rec = (cloud["X"][p].tobytes(), key[p, 1:].tobytes(), cloud["obs_view"][a:b].tobytes(), cloud["obs_pl"][a:b].tobytes(),
               cloud["obs_seg"][a:b].tobytes(), cloud["obs_xy"][a:b].tobytes())
        out.setdefault(int(key[p, 0]), []).append(rec)
    return out


def _task_ids(c, V):
    """per task: (its sample, its V hit lists) as bytes — equal ids = the filter left the task alone"""
    lo = c["list_off"].astype(np.int64)
    ids = []
    for t in range(c["n_tasks"]):
        a, b = int(lo[t * V]), int(lo[(t + 1) * V])
        ids.append((int(c["task_view"][t]), int(c["task_pl"][t]), int(c["task_seg"][t]), c["task_xy"][t].tobytes(),
                    (lo[t * V:(t + 1) * V + 1] - a).tobytes(), c["hit_pl"][a:b].tobytes(), c["hit_seg"][a:b].tobytes(),
                    c["hit_xy"][a:b].tobytes()))
    return ids


class World:
    """One scene + sets + the intervals a PLGMatchesManager would hold (host graph from the ORACLE's replay of the oracle's
    cloud; the device graph from the product's replay of the product's cloud)."""

    def __init__(self, name, scene_ptr, scene_np, sets, make_cloud):
        self.name, self.scene_ptr, self.sets = name, scene_ptr, sets
        ob = _ob()
        self.orc = ob.Oracle(scene_ptr)
        self.S = R.Scene(scene_np, ob.lib())
        self.ctx = api.Context(scene_ptr)
        self.ctx.set_pipelining(1, 0)
        self.graph = self.orc.replay_matches(make_cloud(self.orc))
        self.n_pl = int(scene_np["view_pl_off"][-1])
        self._ref = None
        self.end = sets[0]  # stage A is compared on sets [0, end)

    def ref(self):
        if self._ref is None:
            self._ref = R.stage_a(self.S, *self.sets, self.graph, 0, self.end)
        return self._ref

    def close(self):
        self.ctx.close()
        self.orc.close()


def _synth_world():
    s = host.Synth(0)
    w = World("synth0", s.scene, s.scene_np(), s.polyline_sets(), lambda o: o.match(s.seeds, 0, s.n_seeds, 1))
    w.keep = s
    w.device_cloud = lambda: w.ctx.match_refpoints(s.seeds, device_only=True)
    return w


def _family_world(name):
    case = cases.FAMILIES[name]()
    sa = case.scene_arrays()
    sets = case.csr()
    w = World(name, C.pointer(sa.c), case.scene, sets, lambda o: o.match_polyline_sets(*sets, nthreads=16))
    w.keep = (case, sa)
    w.device_cloud = lambda: w.ctx.match_polyline_sets(*sets, device_only=True)
    if name == "overlap":  # (8 241 samples, which the Python restatement walks at 300 a second: the first 12 of its 46 sets,
        w.end = 12         #  against the intervals of the whole family's cloud — 855 tasks, 1 698 skipped, 2 888 hits dropped)
    return w


WORLDS = {"synth0": _synth_world, "tiny": lambda: _family_world("tiny"), "overlap": lambda: _family_world("overlap"),
          "degenerate": lambda: _family_world("degenerate"), "exact": lambda: _family_world("exact")}


@pytest.fixture(params=sorted(WORLDS))
def world(request, eg3d_form):
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    w = WORLDS[request.param]()
    yield w
    w.close()


# 1 ---- no manager / an empty one: today's path, byte for byte
@pytest.mark.parametrize("name", ["synth0", "tiny"])
def test_no_manager_is_the_plain_call(name, eg3d_form):
    assert api.device_count() >= 1
    w = WORLDS[name]()
    plain = w.ctx.match_polyline_sets(*w.sets)
    assert plain["n_points"] > 0
    _same(plain, w.ctx.match_polyline_sets(*w.sets, matched=_empty_graph(w.n_pl)), (name, "empty manager"))
    e, tm = D.EdgePoints(), D.StageTimes()
    n, row_off, ids = w.sets
    ps = D.PolylineSets(n, D.np_ptr(row_off, C.c_uint32), D.np_ptr(ids, C.c_uint32))
    assert api.lib().eg3d_match_polyline_sets_matched(w.ctx._h, C.byref(ps), 0, n, None, 0, C.byref(e), C.byref(tm)) == 0
    null = D.edgepoints_to_dict(e)
    api.lib().eg3d_free_edgepoints(C.byref(e))
    _same(plain, null, (name, "m = NULL"))
    c0, c1 = w.ctx.polyline_set_candidates(*w.sets), w.ctx.polyline_set_candidates(*w.sets, matched=_empty_graph(w.n_pl))
    assert R.same_candidates(c0, c1) is None and c0["n_samples_skipped"] == 0 and c0["n_hits_filtered"] == 0
    assert R.same_candidates(R.stage_a(w.S, *w.sets, None), c0) is None
    w.close()


# 2 ---- stage A equals the restatement exactly
def test_candidates_equal_the_restatement(world):
    w = world
    ref = w.ref()
    V = w.S.V
    print("%s: %d tasks, %d samples skipped, %d hits filtered (restatement)" % (w.name, ref["n_tasks"], ref["n_samples_skipped"],
                                                                              ref["n_hits_filtered"]))
    # the restatement's own counts: a family that gives 0 proves nothing about that half of the filter
    if w.name in ("synth0", "tiny"):
        assert ref["n_samples_skipped"] > 0 and ref["n_hits_filtered"] > 0, w.name
    elif ref["n_samples_skipped"] == 0 or ref["n_hits_filtered"] == 0:
        print("%s: skipped %d / filtered %d — this family proves nothing about a count of 0" %
              (w.name, ref["n_samples_skipped"], ref["n_hits_filtered"]))
    got = w.ctx.polyline_set_candidates(*w.sets, 0, w.end, matched=w.graph)
    assert R.same_candidates(ref, got) is None, (w.name, "host arrays", R.same_candidates(ref, got))
    # the same with the intervals where eg3d_replay_device left them
    w.device_cloud()
    _, dv, st = w.ctx.replay_device(to_host=False)
    assert int(st["n_intervals"]) == len(w.graph["iv_start_seg"])
    got_d = w.ctx.polyline_set_candidates(*w.sets, 0, w.end, matched=dv)
    assert R.same_candidates(ref, got_d) is None, (w.name, "device arrays", R.same_candidates(ref, got_d))
    if w.name == "tiny":
        rows = R.rows_of(w.graph)
        n, row_off, ids = w.sets
        in_sets = {w.S.gid(r % V, int(p)) for r in range(n * V) for p in ids[row_off[r]:row_off[r + 1]]}
        assert any(g in rows for g in in_sets) and any(g not in rows and len(w.S.vertices(g)) >= 2 for g in in_sets)
        spw = [len(np.unique(ref["task_set"][i:i + 64])) for i in range(0, ref["n_tasks"], 64)]
        assert max(spw) >= 8, ("tiny: the widest wave of 64 tasks spans %d sets" % max(spw))


# 3 ---- end to end: identities against the unfiltered call
@pytest.mark.parametrize("name", ["synth0", "tiny"])
def test_end_to_end_identities(name, eg3d_form):
    assert api.device_count() >= 1
    w = WORLDS[name]()
    V, ctx = w.S.V, w.ctx
    n, row_off, ids = w.sets
    plain, got = ctx.match_polyline_sets(*w.sets), ctx.match_polyline_sets(*w.sets, matched=w.graph)
    cp, cm = ctx.polyline_set_candidates(*w.sets), ctx.polyline_set_candidates(*w.sets, matched=w.graph)
    assert got["n_tasks"] == cm["n_tasks"] == w.ref()["n_tasks"] and plain["n_tasks"] == cp["n_tasks"]
    assert got["flags"] & 7 == 0
    # a task the filter left alone (same sample, same lists) yields byte-identical chains, keys renumbered; a skipped
    # sample yields nothing: every key[0] of the matched cloud is a task of the matched stage A
    where = {tid: i for i, tid in enumerate(_task_ids(cp, V))}
    chains_p, chains_m = _chains(plain), _chains(got)
    assert all(0 <= k < cm["n_tasks"] for k in chains_m)
    alone = 0
    for j, tid in enumerate(_task_ids(cm, V)):
        if tid in where:
            alone += 1
            assert chains_m.get(j) == chains_p.get(where[tid]), (name, "task", j, "plain task", where[tid])
    print("%s: %d of %d tasks untouched by the filter; points %d -> %d" % (name, alone, cm["n_tasks"], plain["n_points"], got["n_points"]))
    assert alone > 0 and got["n_points"] < plain["n_points"]
    # a sub-range = the slice of the whole call
    b, e = max(1, n // 3), max(2, (2 * n) // 3)
    s0 = ctx.polyline_set_candidates(n, row_off, ids, 0, b, matched=w.graph)["n_tasks"]
    s1 = s0 + ctx.polyline_set_candidates(n, row_off, ids, b, e, matched=w.graph)["n_tasks"]
    part = ctx.match_polyline_sets(n, row_off, ids, b, e, matched=w.graph)
    sel = np.nonzero((got["key"][:, 0] >= s0) & (got["key"][:, 0] < s1))[0]
    assert part["n_points"] == len(sel) and part["n_tasks"] == s1 - s0
    if len(sel):
        p0, p1 = int(sel[0]), int(sel[-1]) + 1
        assert p1 - p0 == len(sel)
        o0, o1 = int(got["obs_off"][p0]), int(got["obs_off"][p1])
        key = got["key"][p0:p1].copy()
        key[:, 0] -= np.uint32(s0)
        assert np.array_equal(part["key"], key) and part["X"].tobytes() == got["X"][p0:p1].tobytes()
        assert np.array_equal(part["obs_off"], got["obs_off"][p0:p1 + 1] - np.uint64(o0))
        for k in ("obs_view", "obs_pl", "obs_seg", "obs_xy"):
            assert part[k].tobytes() == got[k][o0:o1].tobytes(), k
    # two lanes, three units = the uncut call, host arrays and device view, host and device intervals
    ctx.set_pipelining(2, 3)
    _same(got, ctx.match_polyline_sets(*w.sets, matched=w.graph), (name, "2 lanes x 3 units"))
    d = ctx.match_polyline_sets(*w.sets, matched=w.graph, device_only=True)
    dev = ctx.fetch_device_output()
    assert d["n_points"] == got["n_points"]
    for k in ARRAYS:
        assert np.ascontiguousarray(dev[k]).tobytes() == np.ascontiguousarray(got[k]).tobytes(), (name, "device view", k)
    ctx.set_pipelining(1, 0)
    w.close()


# 4 ---- nothing left to do
def _cover(S, g):
    """An interval that makes polyline g yield no sample, or None: it starts ON the first vertex of the first sample's
    segment and ends on the last vertex, so the first sample is matched and the jump reaches the end (a first sample on
    segment 0 cannot be matched at all: M1)."""
    v = S.vertices(g)
    if len(v) < 4 or int(S.sc["pl_start"][g]) == int(S.sc["pl_end"][g]):
        return None
    reached, seg, xy = S.next_by_distance(g, v, 0, (v[0][0], v[0][1]))
    if reached or seg < 1 or seg >= len(v) - 2:
        return None
    iv = (seg, (v[seg][0], v[seg][1]), len(v) - 2, (v[-1][0], v[-1][1]))
    return iv


def test_zero_samples_zero_tasks(eg3d_form):
    assert api.device_count() >= 1
    s = host.Synth(0)
    ob = _ob()
    S = R.Scene(s.scene_np(), ob.lib())
    V = S.V
    n, row_off, ids = s.polyline_sets()
    # the sets restricted to the polylines that can be covered
    cover, sets = {}, []
    for i in range(n):
        d = {}
        for v in range(V):
            for p in ids[row_off[i * V + v]:row_off[i * V + v + 1]]:
                iv = _cover(S, S.gid(v, int(p)))
                if iv is not None:
                    cover[S.gid(v, int(p))] = iv
                    d.setdefault(v, []).append(int(p))
        sets.append(d)
    assert sum(1 for d in sets if len(d) >= 3) >= 2, "Synth(0): sets of coverable polylines in three views"
    csr = cases.to_csr(sets, V)
    n_pl = int(S.vpo[-1])

    def graph(gs):
        off, rows = [0], []
        for g in range(n_pl):
            if g in gs:
                rows.append(cover[g])
            off.append(len(rows))
        k = len(rows)
        return {"n_scene_polylines": n_pl, "iv_off": np.asarray(off, np.uint64),
                "iv_start_seg": np.asarray([r[0] for r in rows], np.uint32),
                "iv_start_xy": np.asarray([r[1] for r in rows], np.float32).reshape(k, 2),
                "iv_end_seg": np.asarray([r[2] for r in rows], np.uint32),
                "iv_end_xy": np.asarray([r[3] for r in rows], np.float32).reshape(k, 2)}

    ctx = api.Context(s.scene)
    ctx.set_pipelining(1, 0)
    plain = ctx.match_polyline_sets(*csr)
    assert plain["n_points"] > 0
    # (a) one polyline yields zero samples
    one = sorted(cover)[0]
    ref = R.stage_a(S, *csr, graph({one}))
    v1 = int(np.searchsorted(S.vpo, one, side="right") - 1)
    assert not any(int(ref["task_view"][t]) == v1 and S.gid(v1, int(ref["task_pl"][t])) == one for t in range(ref["n_tasks"]))
    assert ref["n_samples_skipped"] >= 1
    assert R.same_candidates(ref, ctx.polyline_set_candidates(*csr, matched=graph({one}))) is None
    # (b) a set with zero tasks inside a call, alone in a call, (c) a whole call with zero tasks
    set0 = {S.gid(v, p) for v, ps in sets[0].items() for p in ps}
    ref0 = R.stage_a(S, *csr, graph(set0))
    assert not (ref0["task_set"] == 0).any() and ref0["n_tasks"] > 0
    got0 = ctx.match_polyline_sets(*csr, matched=graph(set0))
    assert got0["n_tasks"] == ref0["n_tasks"] and got0["n_points"] > 0
    alone = ctx.match_polyline_sets(csr[0], csr[1], csr[2], 0, 1, matched=graph(set0))
    assert alone["n_points"] == 0 and alone["n_obs"] == 0 and alone["n_tasks"] == 0 and len(alone["X"]) == 0
    everything = graph(set(cover))
    assert R.stage_a(S, *csr, everything)["n_tasks"] == 0
    for lanes, units in ((1, 0), (2, 3)):
        ctx.set_pipelining(lanes, units)
        for device_only in (False, True):
            none = ctx.match_polyline_sets(*csr, matched=everything, device_only=device_only)
            assert none["n_points"] == 0 and none["n_obs"] == 0 and none["n_tasks"] == 0 and none["n_chains"] == 0
    ctx.set_pipelining(1, 0)
    ctx.match_polyline_sets(*csr, matched=everything)
    live = _live()  # (the context's own buffers have their size by now; what is left to vary is what the calls hold)
    assert ctx.match_polyline_sets(*csr, matched=everything)["n_points"] == 0
    c = ctx.polyline_set_candidates(*csr, matched=everything)
    assert c["n_tasks"] == 0 and len(c["list_off"]) == 1 and c["n_samples_skipped"] == len(cover)
    assert _live() == live, "the call's copies of the interval table are released with the call"
    ctx.close()
    s.close()


# 5 ---- the argument checks
def _dev_table(g):
    keep = [api.upload(np.ascontiguousarray(g[k]).reshape(-1) if len(g[k]) else np.zeros(2, np.uint32))
            for k in ("iv_off", "iv_start_seg", "iv_start_xy", "iv_end_seg", "iv_end_xy")]
    m = D.MatchedIntervals(C.sizeof(D.MatchedIntervals), 1, int(g["n_scene_polylines"]), *[a.ptr for a in keep])
    return m, keep


def test_argument_checks_leave_out_untouched(eg3d_form):
    assert api.device_count() >= 1
    case = cases.FAMILIES["degenerate"]()
    sa = case.scene_arrays()
    sc = case.scene
    n, row_off, ids = case.csr()
    ctx = api.Context(C.pointer(sa.c))
    n_pl = int(sc["view_pl_off"][-1])
    nv = np.diff(sc["pl_vtx_off"].astype(np.int64)) * (np.asarray(sc["pl_valid"]) != 0)
    long_g = int(np.nonzero(nv >= 4)[0][0])
    short_g = int(np.nonzero(nv < 2)[0][0])
    v = sc["vtx_xy"][sc["pl_vtx_off"][long_g]:]

    def table(rows, n_scene=n_pl, off=None):
        o, r = [0], []
        for g in range(n_pl):
            r.extend(rows.get(g, ()))
            o.append(len(r))
        k = len(r)
        return {"n_scene_polylines": n_scene, "iv_off": np.asarray(o if off is None else off, np.uint64),
                "iv_start_seg": np.asarray([x[0] for x in r], np.uint32),
                "iv_start_xy": np.asarray([x[1] for x in r], np.float32).reshape(k, 2),
                "iv_end_seg": np.asarray([x[2] for x in r], np.uint32),
                "iv_end_xy": np.asarray([x[3] for x in r], np.float32).reshape(k, 2)}

    p = lambda i: (float(v[i][0]), float(v[i][1]))
    good = {long_g: [(1, p(1), 1, p(2)), (2, p(2), 2, p(3))]}
    nseg = int(nv[long_g]) - 1
    down = table(good)["iv_off"].copy()
    down[long_g + 2] -= 1  # (2, 1, 2: descends, then exceeds nothing)
    bad = {
        "n_scene_polylines": table(good, n_scene=n_pl + 1),
        "offsets not ascending": table(good, off=down),
        "an offset past the total": table(good, off=[0] + [3] * (n_pl - 1) + [2]),
        "start segment outside the polyline": table({long_g: [(nseg, p(1), nseg, p(2))]}),
        "end segment outside the polyline": table({long_g: [(1, p(1), nseg, p(2))]}),
        "start segments not strictly ascending": table({long_g: [(1, p(1), 1, p(2)), (1, p(1), 2, p(3))]}),
        "start segments descending": table({long_g: [(2, p(2), 2, p(3)), (1, p(1), 1, p(2))]}),
        "an interval on a polyline with fewer than two vertices": table({short_g: [(0, (1.0, 1.0), 0, (2.0, 2.0))]}),
    }
    ps = D.PolylineSets(n, D.np_ptr(row_off, C.c_uint32), D.np_ptr(ids, C.c_uint32))
    L = api.lib()

    def call(mc):
        """both entry points with `out` pre-filled: (rc of the match, rc of the candidates), out untouched"""
        e, tm, c = D.EdgePoints(), D.StageTimes(), D.SetCandidates()
        e.n_points, e.flags, c.n_tasks, c.n_hits_filtered = 12345, 0xabcd, 777, 99
        r1 = L.eg3d_match_polyline_sets_matched(ctx._h, C.byref(ps), 0, n, C.byref(mc), 0, C.byref(e), C.byref(tm))
        r2 = L.eg3d_polyline_set_candidates(ctx._h, C.byref(ps), 0, n, C.byref(mc), C.byref(c))
        if r1 != 0:
            assert e.n_points == 12345 and e.flags == 0xabcd and not e.X
        else:
            L.eg3d_free_edgepoints(C.byref(e))
        if r2 != 0:
            assert c.n_tasks == 777 and c.n_hits_filtered == 99 and not c.task_view
        else:
            L.eg3d_free_set_candidates(C.byref(c))
        return r1, r2

    m = D.MatchedIntervalsArrays(table(good))
    assert call(m.c) == (0, 0)
    md, keep = _dev_table(table(good))
    assert call(md) == (0, 0)
    m.c.struct_size -= 4
    assert call(m.c) == (-1, -1), "struct_size"
    for name, g in bad.items():
        assert call(D.MatchedIntervalsArrays(g).c) == (-1, -1), ("host arrays", name)
        md, keep = _dev_table(g)
        assert call(md) == (-1, -1), ("device arrays", name)
        assert b"eg3d_match_polyline_sets_matched" in L.eg3d_last_error()
    ctx.close()


def test_walk_that_does_not_advance_is_refused(eg3d_form):
    """An interval that passes every table check but ends behind the sample it contains (the reference loops for ever):
    EG3D_ERR_ARG from the device walk, as from the host probe and the restatement."""
    assert api.device_count() >= 1
    s = host.Synth(0)
    S = R.Scene(s.scene_np(), _ob().lib())
    V = S.V
    n, row_off, ids = s.polyline_sets()
    chosen = None
    for r in range(n * V):
        for pl in ids[row_off[r]:row_off[r + 1]]:
            if chosen is not None:
                break
            g = S.gid(r % V, int(pl))
            v = S.vertices(g)
            for seg, xy in R.walk(S, r % V, int(pl), None)[0]:
                if seg < 2:
                    continue
                # starts on the first vertex of the sample's segment, ends on the first vertex of the segment BEFORE it
                back = (seg, (v[seg][0], v[seg][1]), seg - 1, (v[seg - 1][0], v[seg - 1][1]))
                try:
                    R.walk(S, r % V, int(pl), [R.Interval(*back)])
                except R.NoProgress:
                    chosen = (r % V, int(pl), g, back, seg, xy)
                    break
    assert chosen is not None, "Synth(0): a sample the jump from the segment before does not get past"
    view, pl, g, back, seg, xy = chosen
    n_pl = int(S.vpo[-1])
    off = np.zeros(n_pl + 1, np.uint64)
    off[g + 1:] = 1
    graph = {"n_scene_polylines": n_pl, "iv_off": off, "iv_start_seg": np.asarray([back[0]], np.uint32),
             "iv_start_xy": np.asarray([back[1]], np.float32), "iv_end_seg": np.asarray([back[2]], np.uint32),
             "iv_end_xy": np.asarray([back[3]], np.float32)}
    with pytest.raises(R.NoProgress):
        R.walk(S, view, pl, R.rows_of(graph)[g])
    # (the walk stalls at the sample itself or, when the jump lands just past it on the same segment, at the landing point,
    # which the same interval holds again: the probe is asked about both)
    _, qseg, qxy = S.next_by_distance(g, S.vertices(g), back[2], back[3])
    with pytest.raises(ValueError, match="do not belong"):
        host.is_matched(s.scene, graph, [view, view], [pl, pl], [seg, qseg], [xy, qxy])
    ctx = api.Context(s.scene)
    for call in (ctx.match_polyline_sets, ctx.polyline_set_candidates):
        with pytest.raises(api.Eg3dError, match="do not belong"):
            call(n, row_off, ids, matched=graph)
    assert ctx.match_polyline_sets(n, row_off, ids)["n_points"] > 0  # the context is fine afterwards
    ctx.close()
    s.close()


# 6 ---- through the reference-API shim (include/eg3d_refapi.hpp)
def test_refapi_manager_and_overload(tmp_path, eg3d_form):
    """tests/refapi/matched_sets_check.cpp on Synth(0): plgmm.is_matched after pipeline 3 agrees with the host probe on the
    midpoint of every segment, and find_new_3d_points_from_compatible_polylines_expandallviews_parallel(sfmd, em, set, plgmm)
    returns, set by set, the points of the C ABI's matched call."""
    import os
    import subprocess
    assert api.device_count() >= 1
    exe = cbuild.build_caller("tests/refapi/matched_sets_check.cpp", tmp_path)  # (links the library of the form under test)
    out = subprocess.run([exe], env=dict(os.environ, EG3D_LIB=""), capture_output=True, text=True, check=True).stdout
    lines = [l.split() for l in out.split("\n") if l]
    s = host.Synth(0)
    ctx = api.Context(s.scene)
    ctx.set_pipelining(1, 0)
    cloud3 = ctx.match_refpoints(s.seeds)
    assert lines[0] == ["R", str(cloud3["n_points"])]
    graph = host.replay_matches(s.scene, cloud3)
    # is_matched
    M = [l for l in lines if l[0] == "M"]
    view, pl, seg = (np.asarray([int(l[i]) for l in M]) for i in (1, 2, 3))
    xy = np.asarray([[int(l[4], 16), int(l[5], 16)] for l in M], np.uint32).view(np.float32)
    k = host.is_matched(s.scene, graph, view, pl, seg, xy)
    assert len(M) > 1000 and (k >= 0).sum() > 0 and (k < 0).sum() > 0
    vpo = s.scene_np()["view_pl_off"].astype(np.int64)
    for i, l in enumerate(M):
        assert int(l[6]) == (1 if k[i] >= 0 else 0), l
        if k[i] >= 0:
            at = int(graph["iv_off"][vpo[view[i]] + pl[i]]) + int(k[i])
            assert (int(l[7]), int(l[8])) == (int(graph["iv_start_seg"][at]), int(graph["iv_end_seg"][at])), l
    # the overload with the filled manager, one call per set
    n, row_off, ids = s.polyline_sets()
    pos = [i for i, l in enumerate(lines) if l[0] == "S"]
    assert [int(lines[i][1]) for i in pos] == list(range(n))
    total = 0
    for c, i in enumerate(pos):
        want = ctx.match_polyline_sets(n, row_off, ids, c, c + 1, matched=graph)
        assert int(lines[i][2]) == want["n_points"], c
        total += want["n_points"]
        j = i + 1
        for p in range(want["n_points"]):
            a, b = int(want["obs_off"][p]), int(want["obs_off"][p + 1])
            assert lines[j][0] == "P" and [int(t, 16) for t in lines[j][1:4]] == [int(t) for t in want["X"][p].view(np.uint32)]
            assert int(lines[j][4]) == b - a
            for o in range(a, b):
                j += 1
                got = lines[j]
                assert got[0] == "O" and [int(got[1]), int(got[2]), int(got[3])] == \
                    [int(want["obs_view"][o]), int(want["obs_pl"][o]), int(want["obs_seg"][o])]
                assert [int(got[4], 16), int(got[5], 16)] == [int(t) for t in want["obs_xy"][o].view(np.uint32)]
            j += 1
    plain = ctx.match_polyline_sets(n, row_off, ids)
    assert 0 < total < plain["n_points"]
    ctx.close()
    s.close()


def test_example_refpoints_first(eg3d_form, tmp_path):
    """examples/edge_matcher_refpoints --refpoints-first on synthetic config 0: pipelines 1-2 find fewer points than in the
    default order (they skip what pipeline 3 matched), and the run with the intervals replayed and read on the device
    (--resident-dedup) writes the JSON of the run with the intervals replayed on the host, byte for byte."""
    import os
    import re
    import subprocess
    import forms
    lib = forms.lib_path(eg3d_form)
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path, lib=lib)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "0", d])
    args = [d + "/input.json", d + "/plgs.bin"]
    stages = ["--all-pairs", "--sets1", d + "/sets1.txt", "--sets2", d + "/sets2.txt"]
    out = {}
    for mode, flags in (("default", []), ("first", ["--refpoints-first"]), ("first_dev", ["--refpoints-first", "--resident-dedup"])):
        path = "%s/%s.json" % (d, mode)
        r = subprocess.run([exe] + args + [path] + stages + flags, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out[mode] = (open(path, "rb").read(), r.stdout)
    pts = {m: [int(x) for x in re.findall(r"pipeline \d: \d+ polyline matches -> (\d+) edge-points", o[1])] for m, o in out.items()}
    print(pts)
    assert len(pts["default"]) == 2 and all(a > b for a, b in zip(pts["default"], pts["first"])), pts
    assert pts["first"] == pts["first_dev"] and "matched intervals (replayed on the device)" in out["first_dev"][1]
    assert "matched intervals (replayed on the host)" in out["first"][1]
    assert out["first"][0] == out["first_dev"][0] and len(out["first"][0]) > 1000
    assert out["first"][1].index("matched ") < out["first"][1].index("pipeline 1:")  # pipeline 3 ran first
