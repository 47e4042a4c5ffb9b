"""Track tables for the triangulation entry points (include/eg3d_triangulate.h, include/eg3d_host_triangulate.h), shared by
tests/test_triangulate_host.py (host statement against the oracle) and tests/test_gpu_triangulate.py (K14 against both). A
table is one call's input: obs_off [n + 1], obs_view, obs_xy, X0 [n, 3]. The requests come from tests/coop_gn_cases.py (rows
that project a true point plus noise, a float start point, and a `kind` that decides how the solve ends); the reference
rows come from the oracle alone: orc_gn_add_batch for EG3D_TRI_REFINE, orc_triangulate (with its `degenerate` flag) for
EG3D_TRI_FROM_SCRATCH. Tracks of fewer than two observations never reach the oracle: the call defines their outcome
(valid = 0, EG3D_TRI_FLAG_SHORT, X_out = X0 or +0.0)."""
import ctypes as C
import functools

import numpy as np

import coop_gn_cases as cg
from edgegraph3d_amd import _cdefs as D

REFINE_KINDS = cg.KINDS
SCRATCH_KINDS = ("near", "wild", "singular", "nan_obs")
FLAG_SHORT, FLAG_DEGENERATE = 1, 2


@functools.lru_cache(maxsize=None)
def rigs():
    return {r.name: r for r in cg.rigs()}


class Table:
    def __init__(self, tracks):
        """tracks: list of dict(view [n], xy [n, 2], X0 [3])"""
        self.n = len(tracks)
        self.obs_off = np.concatenate([[0], np.cumsum([len(t["view"]) for t in tracks])]).astype(np.uint32)
        self.obs_view = np.ascontiguousarray(np.concatenate([np.asarray(t["view"], np.int32) for t in tracks]), np.int32)
        self.obs_xy = np.ascontiguousarray(np.concatenate([np.asarray(t["xy"], np.float32).reshape(-1, 2) for t in tracks]), np.float32)
        self.X0 = np.ascontiguousarray([t["X0"] for t in tracks], np.float32).reshape(-1, 3)
        self.rows = np.diff(self.obs_off.astype(np.int64))

    def args(self):
        return self.obs_off, self.obs_view, self.obs_xy


def short_track(req, n):
    """The first n (0 or 1) rows of a request."""
    return dict(view=req["view"][:n], xy=req["xy"][:n], X0=req["X0"])


def refine_tracks(rig, rng, rows=cg.ROWS, kinds=REFINE_KINDS, long_once=True):
    """Every row count x every kind, 4096 rows once, lengths 0 and 1."""
    out = [cg.make_request(rig, n, kind, rng, has_extra=False) for n in rows for kind in kinds]
    if long_once:
        out.append(cg.make_request(rig, cg.ROWS_LONG_ONLY[0], "far", rng, has_extra=False))
    two = cg.make_request(rig, 2, "near", rng, has_extra=False)
    out += [short_track(two, 0), short_track(two, 1)]
    return out


def dlt_choice_tracks(rig, rng):
    """The three cases of the DLT's choice of entries (triangulate_array: the FIRST entry with the minimal view id, and the
    LAST entry): the minimal view id not at index 0; the minimal view id twice (two different observations of it: taking
    the second changes the start point); the minimal view id in the last entry (degenerate pair, several views in the list)."""
    out = []
    for case in range(3):
        r = cg.make_request(rig, 6, "near", rng, has_extra=False)
        order = np.argsort(r["view"])  # (six distinct views)
        view, xy = r["view"][order].copy(), r["xy"][order].copy()  # ascending: the minimal id at index 0
        if case == 0:
            perm = np.array([3, 1, 0, 2, 5, 4])
        elif case == 1:
            perm = np.array([2, 0, 4, 0, 1, 5])  # index 0 twice, at 1 and 3 ...
        else:
            perm = np.array([1, 2, 3, 4, 5, 0])
        view, xy = view[perm], xy[perm].copy()
        if case == 1:
            xy[3] += np.float32(0.75)  # ... with another observation at the second place
        out.append(dict(view=view, xy=xy, X0=r["X0"]))
    return out


def scratch_tracks(rig, rng, rows=cg.ROWS, long_once=True):
    out = [cg.make_request(rig, n, kind, rng, has_extra=False) for n in rows for kind in SCRATCH_KINDS]
    if long_once:
        out.append(cg.make_request(rig, cg.ROWS_LONG_ONLY[0], "near", rng, has_extra=False))
    out += dlt_choice_tracks(rig, rng)
    two = cg.make_request(rig, 2, "near", rng, has_extra=False)
    out += [short_track(two, 0), short_track(two, 1)]
    return out


@functools.lru_cache(maxsize=None)
def table(rig_name, mode):
    rig = rigs()[rig_name]
    rng = np.random.default_rng(1400 + 10 * sorted(rigs()).index(rig_name) + mode)
    return Table(refine_tracks(rig, rng) if mode == 1 else scratch_tracks(rig, rng))


def oracle_rows(rig, tab, mode):
    """(valid, X, flags) of the call on `tab` as the contract states them, the solves taken from the oracle (in its current
    DLT mode). X is meaningful where valid; elsewhere it is what the call must leave: X0 (mode 1) or +0.0 (mode 0)."""
    from oracle import binding as ob
    n = tab.n
    live = np.nonzero(tab.rows >= 2)[0]
    valid = np.zeros(n, np.uint8)
    flags = np.where(tab.rows < 2, FLAG_SHORT, 0).astype(np.uint8)
    X = tab.X0.copy() if mode == 1 else np.zeros((n, 3), np.float32)
    if mode == 1:
        idx = np.concatenate([np.arange(tab.obs_off[i], tab.obs_off[i + 1]) for i in live]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(tab.rows[live])]).astype(np.uint32)
        v, Xo, _ = ob.gn_add_batch(rig.P, off, tab.obs_view[idx], tab.obs_xy[idx], tab.X0[live])
        valid[live] = v
        ok = live[v != 0]
        X[ok] = Xo[v != 0]
    else:
        L = ob.lib()
        for i in live:
            a, b = int(tab.obs_off[i]), int(tab.obs_off[i + 1])
            ids = np.ascontiguousarray(tab.obs_view[a:b], np.int32)
            xy = np.ascontiguousarray(tab.obs_xy[a:b], np.float32)
            Xi, deg = np.zeros(3, np.float32), C.c_int(0)
            ok = L.orc_triangulate(D.np_ptr(rig.P, C.c_float), ids.ctypes.data_as(C.POINTER(C.c_int)), D.np_ptr(xy, C.c_float),
                                   b - a, D.np_ptr(Xi, C.c_float), C.byref(deg))
            valid[i] = 1 if ok else 0
            if ok:
                X[i] = Xi
            if deg.value:
                flags[i] |= FLAG_DEGENERATE
    return valid, X, flags


def assert_same(got, want, what):
    """valid, flags and X bit for bit. `want` X already holds the contract's value of a track that is not valid."""
    gX, gv, gf = got[:3]
    wv, wX, wf = want
    assert np.array_equal(gv, wv), "%s: valid differs at %s" % (what, np.nonzero(gv != wv)[0][:10])
    if gf is not None:
        assert np.array_equal(gf, wf), "%s: flags differ at %s" % (what, np.nonzero(gf != wf)[0][:10])
    a, b = np.ascontiguousarray(gX, np.float32).view(np.uint32), np.ascontiguousarray(wX, np.float32).view(np.uint32)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert not len(bad), "%s: X differs at %s (valid %s)" % (what, bad[:10], wv[bad[:10]])
