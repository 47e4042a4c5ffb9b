"""-m gpu: eg3d_match_polylines_closeness against the Python restatement of the reference (tests/polymatch_ref.py, pinned
against the oracle by tests/test_polymatch_ref.py). The comparison is exact equality of refpoints, row_off and pl_ids."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cbuild
import polymatch_cases as pc
import polymatch_ref as ref
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host
from oracle import binding as ob
from parity_util import compare_edgepoints

pytestmark = pytest.mark.gpu

_REF = {}   # restatement results, computed once per scene and never modified


def _matcher(name, scene):
    if name not in _REF:
        _REF[name] = ref.Matcher(scene)
    return _REF[name]


def _same(got, want):
    assert got["n_sets"] == want["n_sets"]
    for k in ("refpoints", "row_off", "pl_ids"):
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), (k, got[k], want[k])


def _entries(ctx, n):
    """The test read-back of the per-entry results of the last call (eg3d_polymatch_test_entries)."""
    cnt, pl, dist = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32)
    L = api.lib()
    L.eg3d_polymatch_test_entries.argtypes = [C.c_void_p, C.c_uint32, D.u32p, D.u32p, D.f32p]
    assert L.eg3d_polymatch_test_entries(ctx._h, n, D.np_ptr(cnt, C.c_uint32), D.np_ptr(pl, C.c_uint32),
                                         D.np_ptr(dist, C.c_float)) == 0
    return cnt, pl, dist


def _same_entries(ctx, pts):
    """(count, polyline, distance bits) of every entry against the restatement's search results."""
    want = [r for p in pts for r in p[2]]
    cnt, pl, dist = _entries(ctx, len(want))
    for e, r in enumerate(want):
        assert cnt[e] == len(r), (e, cnt[e], r)
        if r:
            assert pl[e] == r[0][0] and dist[e].tobytes() == np.float32(r[0][1]).tobytes(), (e, pl[e], dist[e], r)


def _hand_scene(name):
    sc, seeds = getattr(pc, name)()
    sa, sd = host.SceneArrays(sc), host.SeedsArrays(*seeds)
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return sc, seeds, sa, sd, api.Context(C.pointer(sa.c))


@pytest.mark.parametrize("name", ["rule_scene", "crowded_scene", "boundary_sample_scene"])
def test_hand_built_scenes(name):
    """Every row of the CPU rule table with real coordinates; observations on 10 px cell boundaries, on and outside the
    image border; a polyline whose samples all fall on a boundary; more than 64 polylines in one window; an invalid
    polyline in the window. The 10 px grid itself is read back and compared too."""
    sc, seeds, sa, sd, ctx = _hand_scene(name)
    with pytest.raises(api.Eg3dError):
        ctx.grid(0, 2)   # not before the first call
    n = len(seeds[0]) - 1
    got = ctx.match_polylines_closeness(C.pointer(sd.c))
    m = _matcher(name, sc)
    want = m.match(seeds, 0, n)
    assert len(want["refpoints"]) >= 1
    _same(got, want)
    _same_entries(ctx, m.entry_results(seeds, 0, n))
    api.check_polyline_sets(got["n_sets"], got["row_off"], got["pl_ids"], sc["n_views"])
    assert got["stats"]["n_entries"] == len(seeds[1]) and got["stats"]["n_accepted"] == len(want["refpoints"])
    assert got["stats"]["n_sets"] == want["n_sets"] and got["stats"]["n_nodes"] == len(want["pl_ids"])
    for v in range(sc["n_views"]):
        ncols, nrows, off, ids = ctx.grid(v, 2)
        g = m.grids[v]
        assert (ncols, nrows) == (g[0], g[1]) and np.array_equal(off, g[2]) and np.array_equal(ids, g[3]), v
    # every seed alone: the verdict of each row of the table, not only their union
    for r in range(n):
        _same(ctx.match_polylines_closeness(None, r, r + 1), m.match(seeds, r, r + 1))
    ctx.close()


def test_rule_table_on_the_device():
    """Every row of the CPU rule table through k9_refpoint_rule itself: the rows are the tracks of one call and their
    hand-made (count, polyline, distance) are fed in place of the search (eg3d_polymatch_test_rule), so the ulp rows, the
    double 0.7 n comparison and the row only `max > 3 min` rejects meet the kernel's arithmetic. Accepted rows, components
    and their order must equal the table's verdicts and the restatement's result."""
    sc, seeds = pc.table_scene()
    sa, sd = host.SceneArrays(sc), host.SeedsArrays(*seeds)
    ctx = api.Context(C.pointer(sa.c))
    ctx.upload_seeds(C.pointer(sd.c))
    rows = pc.RULE_TABLE
    cnt = np.array([len(r) for row in rows for r in row[2]], np.uint32)
    pl = np.array([r[0][0] if r else 0 for row in rows for r in row[2]], np.uint32)
    dist = np.array([r[0][1] if r else 0 for row in rows for r in row[2]], np.float32)
    assert len(cnt) == len(seeds[1])
    L = api.lib()
    L.eg3d_polymatch_test_rule.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, D.u32p, D.u32p, D.f32p, C.POINTER(D.PolylineMatches)]
    m = D.PolylineMatches()
    assert L.eg3d_polymatch_test_rule(ctx._h, 0, len(rows), D.np_ptr(cnt, C.c_uint32), D.np_ptr(pl, C.c_uint32),
                                      D.np_ptr(dist, C.c_float), C.byref(m)) == 0
    acc = D.as_np(m.refpoints, int(m.n_refpoints), np.uint32)
    row_off = D.as_np(m.row_off, int(m.n_sets) * sc["n_views"] + 1, np.uint32)
    got = {"refpoints": acc, "n_sets": int(m.n_sets), "row_off": row_off, "pl_ids": D.as_np(m.pl_ids, int(row_off[-1]), np.uint32)}
    L.eg3d_free_polyline_matches(C.byref(m))
    assert [int(a) for a in acc] == [i for i, row in enumerate(rows) if row[3]]
    _same(got, ref.match_from_results(sc["n_views"], [(i, row[1], row[2]) for i, row in enumerate(rows)]))
    ctx.close()


class Synth:
    def __init__(self, cfg):
        self.s = host.Synth(cfg)
        self.scene = self.s.scene_np()
        self.seeds = self.s.seeds_np()
        self.m = _matcher("config%d" % cfg, self.scene)


def test_config0_whole_and_composition():
    """Synthetic config 0 whole; its sets go straight into eg3d_match_polyline_sets and the cloud equals the oracle's on the
    restatement's sets."""
    y = Synth(0)
    ctx = api.Context(y.s.scene)
    got = ctx.match_polylines_closeness(y.s.seeds)
    want = y.m.match(y.seeds, 0, y.s.n_seeds)
    assert want["n_sets"] >= 3
    _same(got, want)
    _same_entries(ctx, y.m.entry_results(y.seeds, 0, y.s.n_seeds))
    cloud = ctx.match_polyline_sets(got["n_sets"], got["row_off"], got["pl_ids"])
    orc = ob.Oracle(y.s.scene).match_polyline_sets(want["n_sets"], want["row_off"], want["pl_ids"])
    rep = compare_edgepoints(orc, cloud)
    assert rep["ok"], rep["msgs"]
    assert cloud["n_points"] > 0
    ctx.close()


C2_WINDOW = (250, 500)


def test_c2_window():
    """Seeds 250-499 of C2. The restatement says of this window (checked here, on the CPU): 10 accepted points in 9
    components (one component holds the polylines of two accepted points), and rejections by the polyline count, by the
    share of the track and by min < max / 3. No 250-seed window of C2 has a rejection by the last two tests: max > 3 min
    without min < max / 3 needs a rounding edge and fewer than two pairs needs a track of one; the hand-built rule scene
    and the CPU rule table cover them."""
    y = Synth(2)
    b, e = C2_WINDOW
    pts = y.m.entry_results(y.seeds, b, e)
    reasons = [ref.reject_reason(p[1], p[2]) for p in pts]
    assert {"maxpl", "share", "min"} <= set(reasons)
    want = ref.match_from_results(y.scene["n_views"], pts)
    assert want["n_sets"] < len(want["refpoints"])
    ctx = api.Context(y.s.scene)
    ctx.upload_seeds(y.s.seeds)
    _same(ctx.match_polylines_closeness(None, b, e), want)
    _same_entries(ctx, pts)
    ctx.close()


def perturbed_config0():
    """Config 0's seeds with deterministic additions, because no 250-seed window of C2 shows a rejection by every test of
    the rule: for the first accepted point A (track length n), (1) A cut to its first entry (fewer than two pairs), (2) A
    followed by k repeats of its first entry, k the smallest with n < 0.7 (n + k): a view listed again adds to the track but
    not to the distinct pairs (below the share). Config 0 itself has rejections by the polyline count and by min < max / 3.
    A rejection by `max > 3 min` alone needs distances one ulp apart (see the rule table), which pixel coordinates near a
    polyline do not produce: a search over 3000 consecutive floats of one observation and 7 of the other found none; that
    test meets the kernel in test_rule_table_on_the_device."""
    y = Synth(0)
    off, view, xy = [a.copy() for a in y.seeds]
    whole = y.m.match(y.seeds, 0, y.s.n_seeds)
    A = int(whole["refpoints"][0])
    t0, t1 = int(off[A]), int(off[A + 1])
    n = t1 - t0
    k = next(k for k in range(1, 100) if n < 0.7 * (n + k))
    add_view = [view[t0]] + list(view[t0:t1]) + [view[t0]] * k
    add_xy = [xy[t0]] + list(xy[t0:t1]) + [xy[t0]] * k
    off = np.concatenate([off, [off[-1] + 1, off[-1] + 1 + n + k]]).astype(np.uint32)
    return y, (off, np.concatenate([view, add_view]).astype(np.int32),
               np.concatenate([xy, np.array(add_xy, np.float32)]).astype(np.float32))


def test_perturbed_config0_every_reachable_rejection():
    y, seeds = perturbed_config0()
    n = len(seeds[0]) - 1
    pts = y.m.entry_results(seeds, 0, n)
    reasons = [ref.reject_reason(p[1], p[2]) for p in pts]
    assert {"maxpl", "share", "min", "two"} <= set(reasons) and reasons[-2:] == ["two", "share"]
    want = ref.match_from_results(y.scene["n_views"], pts)
    assert want["n_sets"] < len(want["refpoints"])      # a component with the polylines of more than one accepted point
    ctx = api.Context(y.s.scene)
    sd = host.SeedsArrays(*seeds)
    _same(ctx.match_polylines_closeness(C.pointer(sd.c)), want)
    _same_entries(ctx, pts)
    ctx.close()


def _write_sets(path, n_views, r):
    with open(path, "w") as f:
        f.write("eg3d-polyline-sets 1\n%d %d\n" % (r["n_sets"], n_views))
        for k in range(r["n_sets"] * n_views):
            ids = r["pl_ids"][r["row_off"][k]:r["row_off"][k + 1]]
            f.write(" ".join(str(int(x)) for x in [len(ids)] + list(ids)) + "\n")


def test_example_match2_equals_sets2_of_the_restatement(tmp_path):
    """examples/edge_matcher_refpoints.cpp on --make-synthetic scene 2: --match2 writes the JSON the same run writes when
    --sets2 hands it the restatement's sets; both flags together are refused."""
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path, lib=cbuild.DEFAULT_LIB)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "2", d])
    y = Synth(2)
    want = y.m.match(y.seeds, 0, y.s.n_seeds)
    assert want["n_sets"] > 10
    _write_sets(os.path.join(d, "ref_sets2.txt"), y.scene["n_views"], want)
    common = [exe, os.path.join(d, "input.json"), os.path.join(d, "plgs.bin")]
    env = dict(os.environ, EG3D_LIB="")   # (the example links the default library)
    subprocess.check_call(common + [os.path.join(d, "a.json"), "--match2"], env=env)
    subprocess.check_call(common + [os.path.join(d, "b.json"), "--sets2", os.path.join(d, "ref_sets2.txt")], env=env)
    assert open(os.path.join(d, "a.json"), "rb").read() == open(os.path.join(d, "b.json"), "rb").read()
    subprocess.check_call(common + [os.path.join(d, "c.json")], env=env)
    assert open(os.path.join(d, "c.json"), "rb").read() != open(os.path.join(d, "a.json"), "rb").read()
    assert subprocess.call(common + [os.path.join(d, "e.json"), "--match2", "--sets2", os.path.join(d, "ref_sets2.txt")],
                           env=env) == 2


def test_ranges_repeats_and_clones():
    y = Synth(0)
    n = y.s.n_seeds
    ctx = api.Context(y.s.scene)
    ctx.upload_seeds(y.s.seeds)
    empty = ctx.match_polylines_closeness(None, 7, 7)
    assert empty["n_sets"] == 0 and list(empty["row_off"]) == [0] and len(empty["refpoints"]) == 0 and len(empty["pl_ids"]) == 0
    whole = y.m.match(y.seeds, 0, n)
    acc = [int(r) for r in whole["refpoints"]]
    rej = [r for r in range(n) if r not in acc]
    runs = [(a, b) for a in range(n) for b in range(a + 1, n + 1) if not any(a <= r < b for r in acc)]
    a, b = max(runs, key=lambda t: t[1] - t[0])     # the longest range whose points are all rejected
    assert b - a >= 2
    none = ctx.match_polylines_closeness(None, a, b)
    assert none["n_sets"] == 0 and list(none["row_off"]) == [0] and len(none["refpoints"]) == 0
    for (p, q) in ((3, 29), (acc[0], acc[0] + 1), (rej[0], rej[0] + 1), (n // 2, n)):
        _same(ctx.match_polylines_closeness(None, p, q), y.m.match(y.seeds, p, q))
    first = ctx.match_polylines_closeness(None, 0, n)
    clone = ctx.clone()
    assert clone.grid(0, 2)[0] == ctx.grid(0, 2)[0]      # the clone shares the map its parent built
    for c in (ctx, clone):
        again = c.match_polylines_closeness(None, 0, n)
        for k in ("refpoints", "row_off", "pl_ids"):
            assert again[k].tobytes() == first[k].tobytes()
        assert again["stats"]["ms_grid"] == 0.0
    _same(first, whole)
    clone.close()
    ctx.close()


def test_view_id_outside_the_rig():
    y = Synth(0)
    ctx = api.Context(y.s.scene)
    good = ctx.match_polylines_closeness(y.s.seeds)
    off, view, xy = [a.copy() for a in y.seeds]
    view[5] = y.scene["n_views"]
    bad = host.SeedsArrays(off, view, xy)
    m, st = D.PolylineMatches(), D.PolymatchStats()
    st.struct_size = C.sizeof(D.PolymatchStats)
    st.n_entries = 12345
    rc = api.lib().eg3d_match_polylines_closeness(ctx._h, C.pointer(bad.c), 0, len(off) - 1, C.byref(m), C.byref(st))
    assert rc == -1 and b"view id" in api.lib().eg3d_last_error()
    assert not m.row_off and not m.refpoints and m.n_sets == 0 and st.n_entries == 12345
    kept = ctx.match_polylines_closeness(None, 0, y.s.n_seeds)   # the refused seeds did not replace the uploaded ones
    again = ctx.match_polylines_closeness(y.s.seeds)
    for k in ("refpoints", "row_off", "pl_ids"):
        assert np.array_equal(again[k], good[k]) and np.array_equal(kept[k], good[k])
    ctx.close()


def test_refapi_function_equals_the_restatement(tmp_path):
    """polyline_matching_closeness_to_refpoints of include/eg3d_refapi.hpp (tests/refapi/polymatch_check.cpp) on config 1:
    the pair it returns is the restatement's, match by match and view by view."""
    exe = cbuild.build_caller("tests/refapi/polymatch_check.cpp", tmp_path, lib=cbuild.DEFAULT_LIB)
    out = subprocess.run([exe, "1"], env=dict(os.environ, EG3D_LIB=""), capture_output=True, text=True, check=True).stdout
    lines = out.split("\n")
    y = Synth(1)
    want = y.m.match(y.seeds, 0, y.s.n_seeds)
    assert want["n_sets"] >= 2
    assert [int(t) for t in lines[0].split()] == [int(r) for r in want["refpoints"]]
    rows = [[int(t) for t in l.split()] for l in lines[1:1 + want["n_sets"] * y.scene["n_views"]]]
    assert len(lines) == 2 + len(rows)
    for k, row in enumerate(rows):
        assert row == [int(x) for x in want["pl_ids"][want["row_off"][k]:want["row_off"][k + 1]]], k
