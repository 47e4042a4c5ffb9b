"""-m gpu: the matches manager that accumulates over calls on the device (eg3d_replay_accumulate, K8a). Every graph is
compared field for field and bit for bit (replay_gpu_cases.same_graph) with the oracle's replay of the concatenation of the
clouds added so far, and with eg3d_replay_device on the one-call cloud."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import replay_gpu_cases as rc
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host
from oracle import binding as ob
from test_replay_accumulate import chain_starts, concat, parts_at, slice_cloud, _ranges

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_HOSTONLY = -1, -3, -5
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def small():
    sa = rc.small_scene()
    o = ob.Oracle(C.byref(sa.c))
    clouds = rc.cases()
    return sa, o, clouds, {k: o.replay_matches(v) for k, v in clouds.items()}


def _n_pairs(cloud):
    return cloud["n_points"] - 1 - len(chain_starts(cloud)) if cloud["n_points"] else 0


def _check_step(ctx, got, dv, st, want, pairs, what):
    assert rc.same_graph(got, want) is None, (what, rc.same_graph(got, want))
    back = ctx.fetch_device_graph(dv)
    assert rc.same_graph(back, got) is None, (what, "device view", rc.same_graph(back, got))
    assert st["struct_size"] == C.sizeof(D.ReplayStats)
    assert (st["n_pairs"], st["n_nodes"], st["n_polylines"], st["n_intervals"]) == \
        (pairs, want["n_nodes"], want["n_polylines"], int(want["iv_off"][-1])), (what, st)


# ---- 1. hand-built clouds, every subset of their chain boundaries ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_every_cut_of_a_hand_built_cloud(eg3d_form, small, name):
    sa, o, clouds, wants = small
    cloud = clouds[name]
    starts = chain_starts(cloud)
    ctx = api.Context(C.byref(sa.c))
    try:
        for r in range(len(starts) + 1):
            for cuts in itertools.combinations(starts, r):
                parts = parts_at(cloud, cuts)
                if len(parts) > 1:
                    parts = parts[:1] + [slice_cloud(cloud, 0, 0)] + parts[1:]   # an empty cloud in the middle changes nothing
                so_far = []
                for i, p in enumerate(parts):
                    d, held = rc.upload_cloud(ctx, p)
                    got, dv, st = ctx.replay_accumulate(d, reset=(i == 0))
                    so_far.append(p)
                    cat = concat(so_far)
                    _check_step(ctx, got, dv, st, o.replay_matches(cat), _n_pairs(cat), (name, cuts, i))
                    tot = ctx.replay_accumulated()
                    assert (tot["n_points"], tot["n_pairs"]) == (cat["n_points"], _n_pairs(cat))
                assert rc.same_graph(got, wants[name]) is None, (name, cuts)
    finally:
        ctx.close()


# ---- 2. matched clouds in steps ------------------------------------------------------------------------------------------------
_CACHE = {}


class Steps:
    """Per DLT form: synthetic config 0 (whole) and the C2 window of tests/test_gpu_replay_device.py, each with a context
    whose seeds are resident, the one-call cloud, the oracle's graph of it and eg3d_replay_device's."""

    def __init__(self):
        self.items = {}
        for name, cfg, window in (("config0", 0, None), ("c2_window", 2, (1550, 1800))):
            s = host.Synth(cfg)
            ctx = api.Context(s.scene)
            ctx.upload_seeds(s.seeds)
            b, e = (0, s.n_seeds) if window is None else window
            ctx.match_resident(b, e, device_only=True)
            cloud = ctx.fetch_device_output()
            one_shot, _, st = ctx.replay_device()
            self.items[name] = (s, ctx, (b, e), cloud, ob.Oracle(s.scene), one_shot, st)

    def close(self):
        for s, ctx, *_ in self.items.values():
            ctx.close()


def _drop_cache():
    import forms
    for rows, m in list(_CACHE.items()):
        with forms.product_form(rows):
            m.close()
    _CACHE.clear()


@pytest.fixture
def steps(eg3d_form):
    if eg3d_form not in _CACHE:
        _drop_cache()
        _CACHE[eg3d_form] = Steps()
    return _CACHE[eg3d_form]


@pytest.fixture(scope="module", autouse=True)
def _close_cached_contexts():
    yield
    _drop_cache()


@pytest.mark.parametrize("name", ["config0", "c2_window"])
def test_match_steps_accumulate_to_the_one_call_graph(steps, name):
    s, ctx, (b, e), cloud, o, one_shot, st1 = steps.items[name]
    assert rc.same_graph(one_shot, o.replay_matches(cloud)) is None
    for k in (2, 3, 5):
        so_far = []
        for i, (rb, re) in enumerate(_ranges(b, e, k)):
            ctx.match_resident(rb, re, device_only=True)
            so_far.append(ctx.fetch_device_output())
            got, dv, st = ctx.replay_accumulate(None, reset=(i == 0))
            cat = concat(so_far)
            _check_step(ctx, got, dv, st, o.replay_matches(cat), _n_pairs(cat), (name, k, i))
        assert cat["n_points"] == cloud["n_points"]
        assert rc.same_graph(got, one_shot) is None, (name, k, rc.same_graph(got, one_shot))
        assert st["n_pairs"] == st1["n_pairs"]
    # once with the materialisation only at the end
    for i, (rb, re) in enumerate(_ranges(b, e, 5)):
        ctx.match_resident(rb, re, device_only=True)
        got, dv, st = ctx.replay_accumulate(None, reset=(i == 0), materialise=(i == 4))
        assert (got is None and dv is None) == (i < 4)
    _check_step(ctx, got, dv, st, one_shot, st1["n_pairs"], (name, "materialised at the end"))
    assert ctx.replay_accumulated()["state_bytes"] > 0


# ---- 3. the running totals feed the dedup ---------------------------------------------------------------------------------------
def test_totals_are_the_index_base_of_the_dedup(steps):
    s, ctx, (b, e), cloud, o, one_shot, st1 = steps.items["c2_window"]
    ctx.match_resident(b, e, device_only=True)
    keep, n_kept = ctx.dedup_device(ctx.last_device_output())
    whole_mask = keep.numpy(np.uint8)[:cloud["n_points"]]
    masks = []
    for i, (rb, re) in enumerate(_ranges(b, e, 3)):
        ctx.match_resident(rb, re, device_only=True)
        base = 0 if i == 0 else ctx.replay_accumulated()["n_points"]
        dev = ctx.last_device_output()
        keep, _ = ctx.dedup_device(dev, index_base=base, reset=(i == 0))
        masks.append(keep.numpy(np.uint8)[:int(dev.n_points)])
        ctx.replay_accumulate(None, reset=(i == 0), materialise=False)
    assert ctx.replay_accumulated()["n_points"] == cloud["n_points"]
    assert np.array_equal(np.concatenate(masks), whole_mask) and 0 < n_kept < cloud["n_points"]


# ---- 4. state handling ----------------------------------------------------------------------------------------------------------
def test_reset_clone_independence_and_determinism(steps):
    s, ctx, (b, e), cloud, o, one_shot, st1 = steps.items["c2_window"]
    runs = []
    for run in range(2):
        for i, (rb, re) in enumerate(_ranges(b, e, 2)):
            ctx.match_resident(rb, re, device_only=True)
            got, dv, st = ctx.replay_accumulate(None, reset=(i == 0))
            if i == 0:
                first = got
                # an eg3d_replay_device call between two accumulates changes neither result
                mid, dvm, _ = ctx.replay_device()
                assert rc.same_graph(mid, first) is None
                assert rc.same_graph(ctx.fetch_device_graph(dv), first) is None
        assert rc.same_graph(got, one_shot) is None
        assert rc.same_graph(ctx.fetch_device_graph(dvm), first) is None     # ... nor does the accumulate change the replay's
        runs.append((got, ctx.fetch_device_graph(dv)))
    for f in rc.ARRAYS:      # two identical runs are byte-identical
        assert runs[0][0][f].tobytes() == runs[1][0][f].tobytes() == runs[1][1][f].tobytes(), f
    # a clone starts empty, and does not touch its parent's state
    cl = ctx.clone()
    try:
        assert cl.replay_accumulated()["n_points"] == 0
        cl.match_resident(*_ranges(b, e, 2)[1], device_only=True)
        g2, _, _ = cl.replay_accumulate(None)
        assert rc.same_graph(g2, o.replay_matches(cl.fetch_device_output())) is None
        assert ctx.replay_accumulated()["n_points"] == cloud["n_points"]
    finally:
        cl.close()
    # reset: the second half alone
    ctx.match_resident(*_ranges(b, e, 2)[1], device_only=True)
    g3, _, _ = ctx.replay_accumulate(None, reset=True)
    assert rc.same_graph(g3, g2) is None


# ---- 5. refusals leave the state usable -----------------------------------------------------------------------------------------
def _raw(ctx, d, reset=0):
    return api.lib().eg3d_replay_accumulate(ctx._h, C.byref(d), reset, None, None, None)


def test_refusals_leave_the_state_as_it_was(eg3d_form, small):
    sa, o, clouds, wants = small
    ctx = api.Context(C.byref(sa.c))
    try:
        cloud = clouds["c_loop"]
        first, rest = slice_cloud(cloud, 0, 2), slice_cloud(cloud, 2, cloud["n_points"])
        nxt = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in clouds["e_first_interval_wins"].items()}
        nxt["key"] = nxt["key"] + np.array([5, 0, 0, 0], np.uint32)

        def mutated(field, index, value):
            c = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in nxt.items()}
            if field == "X":
                c["X"][index[0], index[1]] = value
            else:
                c[field][index] = value
            return c

        d, held = rc.upload_cloud(ctx, first)
        before, _, _ = ctx.replay_accumulate(d, reset=True)
        assert rc.same_graph(before, o.replay_matches(first)) is None
        nv_p0 = len(rc.POLYLINES[0][rc.P0][0])
        accepted = [first]
        for what, bad, code, reset in (("a cut chain", rest, ERR_ARG, 0),
                                       ("a NaN in a pair", mutated("X", (1, 0), np.nan), ERR_HOSTONLY, 0),
                                       ("x == -1 in a pair, with reset", mutated("X", (0, 0), -1.0), ERR_HOSTONLY, 1),
                                       ("a segment id outside its polyline", mutated("obs_seg", 0, nv_p0 - 1), ERR_ARG, 0)):
            db, heldb = rc.upload_cloud(ctx, bad)
            assert _raw(ctx, db, reset) == code, what
            assert api.lib().eg3d_last_error(), what
            assert ctx.replay_accumulated()["n_points"] == sum(p["n_points"] for p in accepted), what
            # the next valid cloud continues from what was accepted
            step = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in nxt.items()}
            step["key"] = step["key"] + np.array([10 * len(accepted), 0, 0, 0], np.uint32)
            dn, heldn = rc.upload_cloud(ctx, step)
            got, dv, st = ctx.replay_accumulate(dn)
            accepted.append(step)
            cat = concat(accepted)
            _check_step(ctx, got, dv, st, o.replay_matches(cat), _n_pairs(cat), what)
        # the capacity limit, by argument: nothing is read, the check precedes every launch
        big = D.DeviceEdgePoints()
        C.memmove(C.byref(big), C.byref(dn), C.sizeof(big))
        big.n_points = 0xfffffff0 - ctx.replay_accumulated()["n_points"]
        assert _raw(ctx, big) == ERR_CAPACITY
        got, dv, st = ctx.replay_accumulate(rc.upload_cloud(ctx, slice_cloud(cloud, 0, 0))[0])
        _check_step(ctx, got, dv, st, o.replay_matches(cat), _n_pairs(cat), "after the capacity refusal")
    finally:
        ctx.close()


# ---- 6. table growth, in a child process (EG3D_REPLAY_TABLE_BITS is read when a context is created) ---------------------------
def test_table_grows_from_sixteen_slots_in_a_child_process(eg3d_form, steps, tmp_path):
    s, ctx, (b, e), cloud, o, one_shot, st1 = steps.items["c2_window"]
    out = tmp_path / "grown.npz"
    env = dict(os.environ, EG3D_REPLAY_TABLE_BITS="4")
    subprocess.run([sys.executable, os.path.join(HERE, "replay_accumulate_child.py"), str(out)], env=env, check=True, timeout=300)
    z = np.load(out)
    got = {f: (int(z[f]) if f in rc.FIELDS else z[f]) for f in rc.FIELDS + rc.ARRAYS}
    assert rc.same_graph(got, o.replay_matches(cloud)) is None, rc.same_graph(got, one_shot)
    slots, pairs = [int(x) for x in z["slots"]], [int(x) for x in z["pairs"]]
    assert pairs[-1] == st1["n_pairs"] and slots[0] >= 16
    for sl, pr in zip(slots, pairs):      # after every step: the power of two above twice the accumulated pairs
        assert sl == max(16, 1 << (2 * pr).bit_length()), (slots, pairs)
    assert slots[-1] > slots[0]


# ---- 7. the extractor reads the accumulated intervals in place ------------------------------------------------------------------
def test_extractor_reads_the_accumulated_intervals_in_place(steps):
    s, ctx, (b, e), cloud, o, one_shot, st1 = steps.items["c2_window"]
    n_sets, row_off, pl_ids = s.polyline_sets(max_sets=4)
    ctx.match_resident(b, e, device_only=True)
    _, dv1, _ = ctx.replay_device(to_host=False)
    want = ctx.match_polyline_sets(n_sets, row_off, pl_ids, matched=dv1)
    plain = ctx.match_polyline_sets(n_sets, row_off, pl_ids)
    for i, (rb, re) in enumerate(_ranges(b, e, 2)):
        ctx.match_resident(rb, re, device_only=True)
        _, dva, _ = ctx.replay_accumulate(None, reset=(i == 0), to_host=False)
    got = ctx.match_polyline_sets(n_sets, row_off, pl_ids, matched=dva)
    assert got["n_points"] == want["n_points"] > 0
    for f in ("X", "obs_off", "obs_view", "obs_pl", "obs_seg", "obs_xy", "key"):
        assert got[f].tobytes() == want[f].tobytes(), f
    print("extractor: %d points with the manager, %d without" % (want["n_points"], plain["n_points"]))
    assert plain["n_points"] != want["n_points"], "the matched intervals change nothing on these sets: the test would pass vacuously"
