"""-m gpu: the lane-group Gauss-Newton solver of the expand stage (coop_gn_groups, eg3d_dev_coopgn.h) on its own, request by
request, against the oracle's one-lane em_GaussNewton — verdict equal, X bit for bit wherever valid. The windows
(tests/coop_gn_cases.py) are built to reach what whole-pipeline parity only reaches by chance: every packing and group
boundary, long requests of different lengths in one round, more long requests than a round takes, and a spread of
convergence inside one window. Each template instantiation the product runs is checked (TeamWaveT, eg3d_k3b_expand.h), plus
the A/B forms its build switches select. The solver does not depend on the DLT form the suite runs twice for."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

import coop_gn_cases as cg
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api

pytestmark = pytest.mark.gpu

# variant -> (name, has the long-request path) — tests/probe/eg3d_probe.h eg3d_probe_coop_gn
VARIANTS = {0: ("small <0, false, 30>", False), 1: ("general <0, true, 30>", True),
            2: ("many views <EG3D_MANY_KEEP, true, EG3D_GN_PRECHECK_IT>", True),
            3: ("KEEP = 2 <2, true, EG3D_GN_PRECHECK_IT>", True), 4: ("pre-check in general <0, true, EG3D_GN_PRECHECK_IT>", True),
            5: ("pre-check in small <0, false, EG3D_GN_PRECHECK_IT>", False)}


@pytest.fixture(scope="module")
def probe():
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe", "libeg3d_probe.so")
    assert os.path.exists(path), "tests/probe/libeg3d_probe.so is not built (python -m edgegraph3d_amd.build)"
    L = C.CDLL(path)
    L.eg3d_probe_coop_gn.argtypes = [C.c_int, D.f32p, C.c_int, D.i32p, D.f32p, C.c_uint64, C.c_int, D.i32p, D.f32p, C.c_int,
                                     D.u8p, D.f32p, D.i32p, D.u8p]
    assert L.eg3d_probe_coop_gn_variants() == len(VARIANTS)
    return L


@pytest.fixture(scope="module")
def cases():
    """Per rig: the windows, their tables and the oracle's verdict / X / iterations of every request."""
    from oracle import binding as ob
    out = []
    for i, rig in enumerate(cg.rigs()):
        W = cg.build_windows(rig, 1000 + i, n_bulk=800)
        T = W.tables()
        valid, X, iters = ob.gn_add_batch(rig.P, T["row_off"], T["row_view"], T["row_xy"], T["X0"])
        out.append((rig, W, T, dict(valid=valid, X=X, iters=iters, kind=np.array(W.kinds()))))
    return out


def _run(L, variant, rig, W, T):
    nw = len(W.wins)
    ne = nw * cg.REQ
    valid, X, G, refused = np.zeros(ne, np.uint8), np.zeros((ne, 3), np.float32), np.zeros(ne, np.int32), np.zeros(nw, np.uint8)
    rc = L.eg3d_probe_coop_gn(variant, D.np_ptr(rig.P, C.c_float), rig.V, D.np_ptr(T["obs_view"], C.c_int32),
                              D.np_ptr(T["obs_xy"], C.c_float), len(T["obs_view"]), nw, D.np_ptr(T["req_i"], C.c_int32),
                              D.np_ptr(T["req_f"], C.c_float), rig.mid, D.np_ptr(valid, C.c_uint8), D.np_ptr(X, C.c_float),
                              D.np_ptr(G, C.c_int32), D.np_ptr(refused, C.c_uint8))
    assert rc == 0, "eg3d_probe_coop_gn failed (%d)" % rc
    return valid, X, G, refused


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_coop_gn_matches_oracle_bit_for_bit(probe, cases, variant):
    name, long_gn = VARIANTS[variant]
    cov = dict(G=collections.Counter(), Glong=collections.Counter(), rows=collections.Counter(), it=collections.Counter(),
               rejected=0, accepted=0, nonconv_finite=0, refused_windows=0, refused_requests=0, mid=set(), singular=0)
    bad = []
    for rig, W, T, ref in cases:
        valid, X, G, refused = _run(probe, variant, rig, W, T)
        ent = np.flatnonzero(T["req_i"][:, 0])          # entry of request r (the oracle's order)
        n = T["n_req"][ent]
        long_req = n > cg.PACK_MAX
        # the long-request path: refused (never solved) without it, solved with it
        win_long = np.zeros(len(W.wins), bool)
        np.logical_or.at(win_long, ent // cg.REQ, long_req)
        if long_gn:
            assert not refused.any(), [W.names[w] for w in np.flatnonzero(refused)]
        else:
            assert np.array_equal(refused.astype(bool), win_long), [W.names[w] for w in np.flatnonzero(refused != win_long)]
            assert not valid[ent[long_req]].any(), "a refused long request came back valid"
            assert not G[ent[long_req]].any()
            cov["refused_windows"] += int(win_long.sum())
            cov["refused_requests"] += int(long_req.sum())
        solved = ~long_req if not long_gn else np.ones(len(ent), bool)
        v_got, v_ref = valid[ent].astype(bool), ref["valid"].astype(bool)
        # X: the result where valid, and the last iterate of a rejected solve too (the same additions in the same order
        # give the same iterates whatever the verdict) — bit for bit, NaN as NaN (its sign and payload are the chip's)
        x_got, x_ref = X[ent], ref["X"]
        x_same = (x_got.view(np.uint32) == x_ref.view(np.uint32)) | (np.isnan(x_got) & np.isnan(x_ref))
        for r in np.flatnonzero(solved & ~((v_got == v_ref) & x_same.all(1))):
            w, j = divmod(int(ent[r]), cg.REQ)
            bad.append("%s/%s lane %d: n=%d G=%d kind=%s oracle(valid=%d it=%d X=%s) probe(valid=%d X=%s)" % (
                rig.name, W.names[w], j, n[r], G[ent[r]], ref["kind"][r], v_ref[r], ref["iters"][r], ref["X"][r],
                v_got[r], X[ent[r]]))
        s = np.flatnonzero(solved)
        assert (G[ent[s]] >= 2).all() and (G[ent[s]] <= 64).all()
        cov["G"].update(G[ent[s]].tolist())
        cov["Glong"].update(G[ent[s[long_req[s]]]].tolist())
        cov["rows"].update(n[s].tolist())
        it = ref["iters"][s]
        cov["it"].update(np.where(it < 2, "0-1", np.where(it == 2, "2", np.where(it < 30, "3-29", "30"))).tolist())
        finite_in = np.array([np.isfinite(T["row_xy"][T["row_off"][r]:T["row_off"][r + 1]]).all() and
                              np.isfinite(T["X0"][r]).all() for r in s], bool)
        cov["nonconv_finite"] += int(((it == 30) & finite_in).sum())
        cov["singular"] += int((ref["kind"][s] == "singular").sum())
        cov["accepted"] += int(v_ref[s].sum())
        cov["rejected"] += int((~v_ref[s]).sum())
        cov["mid"].add(rig.mid)
    print("\ncoop_gn variant %d (%s): %d requests, accepted %d, rejected %d; oracle iterations (it at the stop): %s, of "
          "which all 30 with finite inputs %d; singular %d; refused long windows %d (%d requests); cams_mid_range %s"
          % (variant, name, sum(cov["G"].values()), cov["accepted"], cov["rejected"], dict(sorted(cov["it"].items())),
             cov["nonconv_finite"], cov["singular"], cov["refused_windows"], cov["refused_requests"], sorted(cov["mid"])))
    print("  G: %s (long requests: %s)" % (dict(sorted(cov["G"].items())), dict(sorted(cov["Glong"].items()))))
    print("  rows: %s" % {k: cov["rows"][k] for k in cg.ROWS + cg.ROWS_LONG_ONLY if cov["rows"][k]})
    assert not bad, "%d of the requests differ from the oracle, e.g.\n  %s" % (len(bad), "\n  ".join(bad[:12]))
    # ---- the test did not pass vacuously
    assert cov["mid"] == {0, 1}
    assert cov["it"]["2"] >= 100 and cov["it"]["3-29"] >= 100 and cov["it"]["30"] >= 20, cov["it"]
    assert cov["nonconv_finite"] >= 5 and cov["singular"] >= 10
    assert cov["accepted"] >= 200 and cov["rejected"] >= 200
    for g in range(2, cg.PACK_MAX + 1):  # short requests: G = the row count
        assert cov["G"][g] >= 3, (g, cov["G"])
    for n in cg.ROWS:
        if n <= cg.PACK_MAX or long_gn:
            assert cov["rows"][n] >= 2, (n, cov["rows"])
    if long_gn:
        assert cov["rows"][4096] >= 2
        for g in (2, 4, 8, 16, 32, 64):  # long requests: powers of two, all of them
            assert cov["Glong"][g] >= 3, (g, cov["Glong"])
    else:
        assert cov["refused_windows"] >= 20 and set(cov["G"]) <= set(range(2, cg.PACK_MAX + 1))
