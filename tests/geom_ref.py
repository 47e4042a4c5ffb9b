"""Reference rows of the tables of tests/geom_cases.py, from the CPU oracle ALONE, computed once per session (reference());
the runners that push the same tables through the host compilation of eg3d_dev_geom.h (tests/hostsim: hostsim_geom_*) or
the gfx950 one (tests/probe: eg3d_probe_walk / _seg / _cells / _closest / _epiline: same arguments); the coverage
conditions, stated on reference rows (and a row mask, so that the GPU test re-asserts them on what it compared); and the
row-by-row comparison with its hex report. Used by tests/test_geom_cases.py (no GPU) and tests/test_gpu_geom_primitives.py.

Rows whose direction is neither end of the polyline are NOT sent to the oracle (undefined in the reference, Q15); their
reference is what the header documents: walk_by_distance -> WALK_EXTREME | WALK_BAD_DIR with out == p, walk_by_line ->
WALK_BAD_DIR with out untouched."""
import ctypes as C
import functools
from types import SimpleNamespace as NS

import numpy as np

import geom_cases as gc
import polymatch_ref as pm
from oracle import binding as ob

f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
u32p, i32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def _f(a):
    return a.ctypes.data_as(f32p)


def _u(a):
    return a.ctypes.data_as(u32p)


def _i(a):
    return a.ctypes.data_as(i32p)


def _b(a):
    return a.ctypes.data_as(u8p)


def _sent_u(n):
    return np.full(n, gc.SENT_U32, np.uint32)


def _sent_f(shape):
    return np.full(shape, gc.SENT_F32, np.float32)


WALK_FORMS = {0: "walk_by_distance", 1: "walk_by_distance_pf", 2: "walk_by_line", 3: "walk_by_line<lds>", 4: "walk_by_line_pf",
              5: "head<1>+body+resolve", 6: "head<2>+body+resolve", 7: "head<3>+body+resolve", 8: "head<4>+body+resolve"}
DISTANCE_FORMS, LINE_FORMS, LDS_FORM = (0, 1), (2, 3, 4, 5, 6, 7, 8), 3
SEG_HIT, SEG_GUARDED, SEG_PLDIST, SEG_COS_GT = 0, 1, 2, 3
CELL_OF, CELL_WINDOW = 0, 1
CLOSEST_WHOLE, CLOSEST_RANGE, CLOSEST_PRUNED = 0, 1, 2


def bind(L, prefix):
    """argtypes of the five table entry points of libhostsim.so (prefix hostsim_geom_) / libeg3d_probe.so (eg3d_probe_)"""
    g = lambda name: getattr(L, prefix + name)
    g("walk").argtypes = [C.c_int, f32p, C.c_uint64, u32p, u32p, u32p, C.c_uint32, C.c_uint64, u32p, u32p, u32p, f32p, u8p, u32p,
                          u32p, f32p]
    g("seg").argtypes = [C.c_int, C.c_uint64, f32p, u32p, f32p]
    g("cells").argtypes = [C.c_int, C.c_uint64, f32p, i32p, i32p]
    g("closest").argtypes = [C.c_int, f32p, C.c_uint64, u32p, C.c_uint32, f32p, C.c_uint64, u32p, C.c_uint64, u32p, u32p, u32p,
                             f32p, f32p, u32p, f32p]
    g("epiline").argtypes = [C.c_uint64, f64p, u8p, f32p, i32p, f32p]
    return NS(walk=g("walk"), seg=g("seg"), cells=g("cells"), closest=g("closest"), epiline=g("epiline"))


# ---------------------------------------------------------------- runners (hostsim or probe: `E` = bind(...)) ----
def run_walk(E, form, rows=None):
    """status, seg, xy [n][2] over the sentinel; rows = an index array (ascending) or None for all"""
    w = gc.walk_table()
    idx = np.arange(w.n) if rows is None else np.asarray(rows)
    rp, rs, rd = (np.ascontiguousarray(a[idx]) for a in (w.row_pl, w.row_seg, w.row_dir))
    rf, rb = np.ascontiguousarray(w.row_f[idx]), np.ascontiguousarray(w.row_bnd[idx])
    n = len(idx)
    st, sg, xy = _sent_u(n), _sent_u(n), _sent_f((n, 2))
    rc = E.walk(form, _f(w.vtx), w.nv, _u(w.pl_off), _u(w.pl_start), _u(w.pl_end), w.npl, n, _u(rp), _u(rs), _u(rd), _f(rf), _b(rb),
                _u(st), _u(sg), _f(xy))
    assert rc == 0, ("walk form %d" % form, rc)
    return NS(status=st, seg=sg, xy=xy)


def run_seg(E, mode, rows):
    n = len(rows)
    r, o = _sent_u(n), _sent_f((n, 2))
    rc = E.seg(mode, n, _f(rows), _u(r), _f(o))
    assert rc == 0, ("seg mode %d" % mode, rc)
    return NS(r=r, o=o)


def run_cells(E, mode):
    t = gc.cell_table()
    rows, dims = (t.rows, t.dims) if mode == CELL_OF else (t.wrows, t.wdims)
    out = np.full((len(rows), 4), gc.SENT_I32, np.int32)
    rc = E.cells(mode, len(rows), _f(rows), _i(dims), _i(out))
    assert rc == 0, ("cells mode %d" % mode, rc)
    return out


def run_closest(E, mode):
    t = gc.closest_table()
    d, sg, xy = _sent_f(t.n), _sent_u(t.n), _sent_f((t.n, 2))
    rc = E.closest(mode, _f(t.vtx), t.nv, _u(t.pl_off), t.npl, _f(t.bb), len(t.bb), _u(t.bb_off), t.n, _u(t.row_pl), _u(t.row_s0),
                   _u(t.row_s1), _f(t.q), _f(d), _u(sg), _f(xy))
    assert rc == 0, ("closest mode %d" % mode, rc)
    return NS(d=d, seg=sg, xy=xy)


def run_epiline(E, t):
    ok, line = np.full(t.n, gc.SENT_I32, np.int32), _sent_f((t.n, 3))
    rc = E.epiline(t.n, t.F.ctypes.data_as(f64p), _b(t.valid), _f(t.xy), _i(ok), _f(line))
    assert rc == 0, rc
    return NS(ok=ok, line=line)


# ---------------------------------------------------------------- the reference ----
def epiline_cases():
    """the table on the F matrices of two synthetic rigs (host.Synth(0), host.Synth(1))"""
    if "epi" not in gc._CACHE:
        from edgegraph3d_amd import host
        Fs = []
        for cfg in (0, 1):
            s = host.Synth(cfg)
            sc = s.scene_np()
            F = sc["F"].reshape(-1, 9)[sc["F_valid"].reshape(-1) != 0]
            Fs.append(F[:: max(1, len(F) // 5)][:5].copy())
        gc._CACHE["epi"] = gc.epiline_table(Fs)
    return gc._CACHE["epi"]


def _ref_walks(L):
    w = gc.walk_table()
    ends = np.flatnonzero(w.row_dirkind != gc.DIR_NEITHER)
    bad = np.flatnonzero(w.row_dirkind == gc.DIR_NEITHER)
    rp, rs, rd = (np.ascontiguousarray(a[ends]) for a in (w.row_pl, w.row_seg, w.row_dir))
    f = w.row_f[ends]
    n = len(ends)
    # next_pl_point_by_distance
    dist = NS(status=_sent_u(w.n), seg=_sent_u(w.n), xy=_sent_f((w.n, 2)))
    st, sg, xy = _sent_u(n), _sent_u(n), _sent_f((n, 2))
    xyd = np.ascontiguousarray(f[:, [0, 1, 5]])
    L.orc_batch_next_by_distance(_f(w.vtx), _u(w.pl_off), _u(w.pl_start), _u(w.pl_end), n, _u(rp), _u(rs), _u(rd), _f(xyd), _u(st),
                                 _u(sg), _f(xy))
    dist.status[ends], dist.seg[ends], dist.xy[ends] = st, sg, xy
    dist.status[bad] = gc.WALK_EXTREME | gc.WALK_BAD_DIR       # the header's documented result: out == p
    dist.seg[bad] = w.row_seg[bad]
    dist.xy[bad] = w.row_f[bad, 0:2]
    # next_pl_point_by_line_intersection(_bounded_distance)
    line = NS(status=_sent_u(w.n), seg=_sent_u(w.n), xy=_sent_f((w.n, 2)))
    st, sg, xy = _sent_u(n), _sent_u(n), _sent_f((n, 2))
    pxy, ln, mm = (np.ascontiguousarray(f[:, c]) for c in ([0, 1], [2, 3, 4], [6, 7]))
    rb = np.ascontiguousarray(w.row_bnd[ends])
    L.orc_batch_next_by_line(_f(w.vtx), _u(w.pl_off), _u(w.pl_start), _u(w.pl_end), n, _u(rp), _u(rs), _u(rd), _f(pxy), _f(ln),
                             _b(rb), _f(mm), _u(st), _u(sg), _f(xy))
    line.status[ends], line.seg[ends], line.xy[ends] = st, sg, xy
    line.status[bad] = gc.WALK_BAD_DIR                        # out untouched: the sentinel stays
    return dist, line


def _ref_segs(L):
    t = gc.seg_table()

    def one(rows):
        n = len(rows)
        r7 = np.ascontiguousarray(rows[:, :7])
        found, fn, qp = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        inter, intern, dist = _sent_f((n, 2)), _sent_f((n, 2)), np.zeros(n, np.float32)
        L.orc_batch_segment_line(n, _f(r7), _b(found), _f(inter), _b(fn), _f(intern), _b(qp), _f(dist))
        cos = np.zeros(n, np.float32)
        L.orc_batch_anglecos(n, _f(r7), _f(cos))
        return NS(found=found, inter=inter, found_nqp=fn, inter_nqp=intern, qp=qp, dist=dist, cos=cos)

    s, p = one(t.rows), one(t.points)
    # a zero-length segment has den == 0: the reference takes the distance branch, distance_point_line of (x1, y1)
    assert (p.found_nqp == 0).all() and (p.dist >= 0).all()
    return NS(hit=NS(r=s.found.astype(np.uint32), o=s.inter),
              guarded=NS(r=s.found_nqp.astype(np.uint32) | (s.qp.astype(np.uint32) << 1), o=s.inter_nqp),
              cos=s.cos, pldist=p.dist)


def _ref_cells(L):
    t = gc.cell_table()
    of = np.zeros((t.n, 4), np.int32)
    L.orc_batch_cell_from_coords(t.n, _f(t.rows), _i(of))
    cw = np.zeros((t.m, 4), np.int32)
    L.orc_batch_cell_from_coords(t.m, _f(t.wrows), _i(cw))
    win = np.zeros((t.m, 4), np.int32)
    for k in range(t.m):
        iw, ih, mw, mh = (int(v) for v in t.wdims[k])
        r = pm.window_rule(iw, ih, mw, mh, t.wrows[k, 1], t.wrows[k, 2], (int(cw[k, 0]), int(cw[k, 1]), bool(cw[k, 2]), bool(cw[k, 3])))
        win[k] = (0, -1, 0, -1) if r is None else r    # (c0 c1 r0 r1; the empty window as cell_window spells it)
    return NS(of=of, window=win, window_cell=cw)


def _ref_closest(L):
    """per (polyline, range): orc_batch_mindist of every (query, segment), then the scan — the first segment of a range that
    starts at 0 is the initial best (NaN included: a NaN best is never replaced), later ones replace it when STRICTLY
    smaller; a range that starts later begins from +inf with seg = 0xffffffff and the point (0, 0)."""
    t = gc.closest_table()
    d, sg, xy = np.zeros(t.n, np.float32), np.zeros(t.n, np.uint32), np.zeros((t.n, 2), np.float32)
    ties_far, ties_any = np.zeros(t.n, bool), np.zeros(t.n, bool)
    key = t.row_pl.astype(np.int64) * (1 << 40) + t.row_s0.astype(np.int64) * (1 << 20) + t.row_s1
    with np.errstate(invalid="ignore"):
        for kv in np.unique(key):
            idx = np.flatnonzero(key == kv)
            p, s0, s1 = int(t.row_pl[idx[0]]), int(t.row_s0[idx[0]]), int(t.row_s1[idx[0]])
            v = t.vtx[t.pl_off[p]:t.pl_off[p + 1]]
            q = t.q[idx]
            m = len(idx)
            best, bs, bxy = np.full(m, np.inf, np.float32), np.full(m, 0xffffffff, np.uint32), np.zeros((m, 2), np.float32)
            cols = []
            for i in range(s0, s1):
                pvw = np.ascontiguousarray(np.concatenate([q, np.tile(np.concatenate([v[i], v[i + 1]]), (m, 1))], 1), np.float32)
                out = np.zeros((m, 3), np.float32)
                L.orc_batch_mindist(m, _f(pvw), _f(out))
                cols.append(out[:, 0].copy())
                take = np.ones(m, bool) if (i == 0 and s0 == 0) else out[:, 0] < best
                best[take], bs[take], bxy[take] = out[take, 0], i, out[take, 1:3]
            d[idx], sg[idx], xy[idx] = best, bs, bxy
            if cols:
                dm = np.stack(cols, 1)
                eq = dm == best[:, None]
                ties_any[idx] = eq.sum(1) >= 2
                first = np.argmax(eq, 1)
                last = dm.shape[1] - 1 - np.argmax(eq[:, ::-1], 1)
                ties_far[idx] = eq.any(1) & (last - first >= 2)
    return NS(d=d, seg=sg, xy=xy, ties_any=ties_any, ties_far=ties_far)


def _ref_epiline(L):
    t = epiline_cases()
    ok, line = np.full(t.n, gc.SENT_I32, np.int32), _sent_f((t.n, 3))
    L.orc_batch_epiline(t.n, t.F.ctypes.data_as(f64p), _b(t.valid), _f(t.xy), _i(ok), _f(line))
    return NS(ok=ok, line=line)


@functools.lru_cache(maxsize=None)
def reference():
    """every table's reference rows, once per session"""
    L = ob.lib()
    dist, line = _ref_walks(L)
    return NS(walk_dist=dist, walk_line=line, seg=_ref_segs(L), cells=_ref_cells(L), closest=_ref_closest(L), epiline=_ref_epiline(L))


# ---------------------------------------------------------------- comparison ----
def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def _hex(v):
    v = np.atleast_1d(v)
    return "[" + " ".join("%s=%#x" % (repr(float(x)) if v.dtype.kind == "f" else int(x), int(_bits(np.array([x], v.dtype))[0]) & 0xffffffffffffffff)
                          for x in v) + "]"


def differing_rows(ref, got):
    """ref / got: dicts name -> array with the rows first. Bits of floats are compared, except that NaN equals NaN; the
    sign of zero counts. Returns the indices of the rows that differ in any field."""
    bad = None
    for name in ref:
        a, b = np.asarray(ref[name]), np.asarray(got[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        ne = _bits(a) != _bits(b)
        if a.dtype.kind == "f":
            ne &= ~(np.isnan(a) & np.isnan(b))
        ne = ne.reshape(len(a), -1).any(1)
        bad = ne if bad is None else (bad | ne)
    return np.flatnonzero(bad)


def assert_rows_equal(what, ref, got, inputs):
    """zero differing rows, or the first dozen with inputs, reference and result in hex"""
    bad = differing_rows(ref, got)
    if len(bad):
        lines = []
        for k in bad[:12]:
            lines.append("row %d: in %s\n      ref %s\n      got %s" % (
                k, " ".join("%s%s" % (n, _hex(np.asarray(a)[k])) for n, a in inputs.items()),
                " ".join("%s%s" % (n, _hex(np.asarray(a)[k])) for n, a in ref.items()),
                " ".join("%s%s" % (n, _hex(np.asarray(a)[k])) for n, a in got.items())))
        raise AssertionError("%s: %d of %d rows differ from the reference, e.g.\n  %s" % (what, len(bad), len(next(iter(ref.values()))),
                                                                                         "\n  ".join(lines)))


def walk_inputs(rows=None):
    w = gc.walk_table()
    idx = slice(None) if rows is None else rows
    return {"pl": w.row_pl[idx], "n": w.row_size[idx], "seg": w.row_seg[idx], "dir": w.row_dirkind[idx], "bnd": w.row_bnd[idx],
            "f": w.row_f[idx]}


# ---------------------------------------------------------------- coverage conditions (on reference rows) ----
def walk_coverage(ref_dist=None, ref_line=None, rows=None):
    """The floors of the walk tables on the reference rows `rows` (None: all). A size's rows must show every status the
    size can produce: ALL FIVE for every size, two vertices included — but a 2-vertex polyline produces them from the
    partial segment at the start point only: it has no whole segment ahead (from 3 vertices on) and no continuation past
    a head of four whole segments (from 7 vertices on), so those two conditions start at the sizes that can meet them."""
    w = gc.walk_table()
    sel = np.zeros(w.n, bool)
    sel[np.arange(w.n) if rows is None else rows] = True
    F, E, Q, B, X = gc.WALK_FOUND, gc.WALK_EXTREME, gc.WALK_QUASIPARALLEL, gc.WALK_BOUND, gc.WALK_BAD_DIR
    bnd = w.row_bnd != 0
    if ref_dist is not None:
        st = ref_dist.status
        for dk in (gc.DIR_START, gc.DIR_END):
            for s in (F, E):
                n = int((sel & (w.row_dirkind == dk) & (st == s)).sum())
                assert n >= 100, ("walk_by_distance", dk, s, n)
        assert int((sel & (st == (E | X))).sum()) >= 100
        for size in gc.SIZES:
            got = set(int(s) for s in np.unique(st[sel & (w.row_size == size)]))
            assert got >= {F, E, E | X}, ("walk_by_distance", size, got)
            if size >= 3:   # a hit beyond the partial segment
                assert (sel & (w.row_size == size) & (st == F) & (ref_dist.seg != w.row_seg)).any(), size
    if ref_line is not None:
        st = ref_line.status
        for dk in (gc.DIR_START, gc.DIR_END):
            for b in (False, True):
                for s in (F, E, Q) + ((B,) if b else ()):
                    n = int((sel & (w.row_dirkind == dk) & (bnd == b) & (st == s)).sum())
                    assert n >= 100, ("walk_by_line", dk, b, s, n)
        for b in (False, True):
            assert int((sel & (bnd == b) & (st == X)).sum()) >= 100
        assert not (sel & ~bnd & (st == B)).any()
        hit = (st == F) | (st == B)
        far = np.abs(ref_line.seg.astype(np.int64) - w.row_seg.astype(np.int64))
        for size in gc.SIZES:
            m = sel & (w.row_size == size)
            got = set(int(s) for s in np.unique(st[m]))
            assert got >= {F, E, Q, B, X}, ("walk_by_line", size, got)
            if size >= 3:
                assert (m & hit & (far >= 1)).any(), size
            if size >= 7:   # decided past the head's window of four whole segments: the body / the shifts of the window
                assert (m & hit & (far >= 5)).any(), size
        # the bound family: hits on both sides of every bound, within 1e-3 of it
        d = np.sqrt(((ref_line.xy.astype(np.float64) - w.row_f[:, 0:2]) ** 2).sum(1))
        fam = sel & (w.row_fam == gc.FAM_BOUND) & hit
        for bound in sorted({5.0, 15.0, gc.FOLLOW_MIN, gc.FOLLOW_MAX}):
            lo = int((fam & (d < bound) & (d > bound - 1e-3)).sum())
            hi = int((fam & (d > bound) & (d < bound + 1e-3)).sum())
            assert lo >= 20 and hi >= 20, ("bound", bound, lo, hi)
        for (mn, mx) in gc.WINDOWS:
            inwin = fam & (w.row_f[:, 6] == np.float32(mn)) & (w.row_f[:, 7] == np.float32(mx))
            assert (inwin & (st == F)).sum() >= 20 and (inwin & (st == B)).sum() >= 20, (mn, mx)


def qp_band_coverage(ref, rows=None):
    """the 0.965 family straddles its edge: reference cosines on each side of it, within 2e-4"""
    t = gc.seg_table()
    sel = np.zeros(t.n, bool)
    sel[np.arange(t.n) if rows is None else rows] = True
    qp = sel & (t.fam == gc.FAM_QP)
    above = int((qp & (ref.cos > gc.QP_COS) & (ref.cos < gc.QP_COS + gc.QP_BAND)).sum())
    below = int((qp & (ref.cos <= gc.QP_COS) & (ref.cos > gc.QP_COS - gc.QP_BAND)).sum())
    assert above >= 50 and below >= 50, (above, below)


def seg_coverage(ref, rows=None):
    t = gc.seg_table()
    sel = np.zeros(t.n, bool)
    sel[np.arange(t.n) if rows is None else rows] = True
    r = t.rows
    qp_band_coverage(ref, rows)
    # hit parameter exactly 0 (the hit is the first vertex) or exactly 1 (the hit is x1 + (x2 - x1), rounded)
    found = sel & (ref.hit.r == 1)
    t0 = found & (_bits(ref.hit.o[:, 0]) == _bits(r[:, 0])) & (_bits(ref.hit.o[:, 1]) == _bits(r[:, 1]))
    e = np.stack([r[:, 0] + (r[:, 2] - r[:, 0]), r[:, 1] + (r[:, 3] - r[:, 1])], 1).astype(np.float32)
    t1 = found & ~t0 & (ref.hit.o[:, 0] == e[:, 0]) & (ref.hit.o[:, 1] == e[:, 1]) & (t.fam == gc.FAM_VERTEX)
    assert int(t0.sum()) >= 50 and int(t1.sum()) >= 50, (int(t0.sum()), int(t1.sum()))
    # every outcome of the guarded test, the zero-length and the degenerate rows included
    for v in (0, 1, 2, 3):
        assert int((sel & (ref.guarded.r == v)).sum()) >= 50, v
    for fam in (5, 6):
        assert len(set(ref.guarded.r[sel & (t.fam == fam)].tolist())) >= 2, fam
    with np.errstate(over="ignore", invalid="ignore"):
        ax, ay = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
        by = np.where(r[:, 5] == 0, np.float32(1), -r[:, 4] / np.where(r[:, 5] == 0, np.float32(1), r[:, 5]))
        bx = np.where(r[:, 5] == 0, np.float32(0), np.float32(1))
        prod = (ax * ax + ay * ay) * (bx * bx + by * by)
        # rows on which the comparison of squares ALONE (no margin, no re-evaluation) would decide differently from the
        # reference cosine: what the 1e-4 band of seg_line_cos_gt exists for
        d = ax * bx + ay * by
        thr = gc.QP_COS
        d2, rhs = d * d, (thr * thr) * prod
        mid = sel & (prod > np.float32(1e-30)) & (prod < np.float32(1e30)) & (d > 0)
        sq_yes = int((mid & (d2 > rhs) & (ref.cos <= thr)).sum())
        on_edge = int((sel & (ref.cos == thr)).sum())
    # (the opposite disagreement, squares say no and the cosine says yes, is rare with this threshold — a handful of rows of
    # this table — and no floor is set for it)
    assert sq_yes >= 20 and on_edge >= 20, (sq_yes, on_edge)
    assert int((sel & (prod <= np.float32(1e-30))).sum()) >= 100 and int((sel & (prod >= np.float32(1e30))).sum()) >= 100
    assert int((sel & (prod == 0) & ((ax != 0) | (ay != 0))).sum()) >= 20 and int((sel & np.isinf(prod)).sum()) >= 20


def cell_coverage(ref, rows=None):
    t = gc.cell_table()
    sel = np.zeros(t.n, bool)
    sel[np.arange(t.n) if rows is None else rows] = True
    # the band family: consecutive floats (runs of 17, one ulp apart) that fall into different cells / flags
    for cell in gc.CELLS:
        for (col, tag, out) in ((1, t.tag_x, 0), (2, t.tag_y, 1)):
            m = np.flatnonzero(sel & (t.rows[:, 0] == cell) & (tag == 3))
            v, c = t.rows[m, col], ref.of[m, out]
            order = np.argsort(v, kind="stable")
            v, c = v[order], c[order]
            one_ulp = np.nextafter(v[:-1], np.float32(np.inf)) == v[1:]
            assert int((one_ulp & (c[1:] == c[:-1] + 1)).sum()) >= 30, (cell, col)
    for k in (2, 3):
        assert set(ref.of[sel, k].tolist()) == {0, 1}
    assert (ref.of[sel, 0] < 0).any() and (ref.of[sel, 0] > 100000).any()


def window_coverage(ref, rows=None):
    t = gc.cell_table()
    sel = np.zeros(t.m, bool)
    sel[np.arange(t.m) if rows is None else rows] = True
    w = ref.window
    empty = w[:, 1] < w[:, 0]
    assert int((sel & empty).sum()) >= 50 and int((sel & ~empty).sum()) >= 1000
    cw = ref.window_cell
    past = sel & ~empty & ((cw[:, 0] >= t.wdims[:, 2]) | (cw[:, 1] >= t.wdims[:, 3]))      # the "compares as unsigned" branch
    last = sel & ~empty & ((cw[:, 0] == t.wdims[:, 2] - 1) | (cw[:, 1] == t.wdims[:, 3] - 1))
    first = sel & ~empty & ((cw[:, 0] == 0) | (cw[:, 1] == 0))
    assert int(past.sum()) >= 100 and int(last.sum()) >= 100 and int(first.sum()) >= 100
    widths = set((w[sel & ~empty, 1] - w[sel & ~empty, 0]).tolist()) | set((w[sel & ~empty, 3] - w[sel & ~empty, 2]).tolist())
    assert widths >= {0, 1, 2}, widths


def whole_range_rows():
    """the rows of the closest-point table whose range is the whole polyline: what polyline_closest (no range) is compared on"""
    t = gc.closest_table()
    nseg = (t.pl_off[1:] - t.pl_off[:-1] - 1)[t.row_pl]
    return np.flatnonzero((t.row_s0 == 0) & (t.row_s1 == nseg))


def closest_coverage(ref, rows=None, ranges=True):
    t = gc.closest_table()
    sel = np.zeros(t.n, bool)
    sel[np.arange(t.n) if rows is None else rows] = True
    assert int((sel & ref.ties_far).sum()) >= 50 and int((sel & ref.ties_any).sum()) >= 50   # ties between different segments
    assert int((sel & np.isnan(ref.d)).sum()) >= 20 and int((sel & (ref.d == 0)).sum()) >= 50
    if ranges:   # empty ranges and ranges from segment 1 on that find nothing finite
        assert int((sel & (ref.seg == 0xffffffff)).sum()) >= 100
        assert int((sel & (t.row_s0 == 1)).sum()) >= 100 and int((sel & (t.row_s0 % gc.BB_SEGS != 0)).sum()) >= 100


def epiline_coverage(ref, rows=None):
    t = epiline_cases()
    sel = np.zeros(t.n, bool)
    sel[np.arange(t.n) if rows is None else rows] = True
    for k in range(5):
        assert int((sel & (t.kind == k)).sum()) >= 50, k
    assert (ref.ok[sel & (t.kind == 3)] == 0).all() and (ref.ok[sel & (t.kind != 3)] == 1).all()
    norm = np.hypot(ref.line[:, 0].astype(np.float64), ref.line[:, 1])
    assert (np.abs(norm[sel & (t.kind < 3)] - 1) < 1e-6).all() and (norm[sel & (t.kind == 4)] == 0).all()


# ---------------------------------------------------------------- checks both halves share ----
def check_cos_gt(ref, got, t):
    """seg_line_cos_gt == the plain comparison on every row; == orc_batch_anglecos > 0.965f wherever the oracle's cosine is
    not NaN; and seg_line_cos itself equals the oracle's cosine"""
    fast, plain = got.r & 1, (got.r >> 1) & 1
    inp = {"row": t.rows, "cos": ref.cos}
    assert_rows_equal("seg_line_cos_gt against seg_line_cos(...) > thr", {"gt": plain}, {"gt": fast}, inp)
    assert_rows_equal("seg_line_cos", {"cos": ref.cos}, {"cos": got.o[:, 0].copy()}, inp)
    ok = np.flatnonzero(~np.isnan(ref.cos))
    assert 1000 <= len(ref.cos) - len(ok) <= len(ref.cos) // 4   # (0 / 0: the zero-length segments, e.g. from a start point on a vertex)
    want = (ref.cos > gc.QP_COS).astype(np.uint32)
    assert_rows_equal("seg_line_cos_gt against the oracle's cosine", {"gt": want[ok]}, {"gt": fast[ok]},
                         {k: v[ok] for k, v in inp.items()})
    qp_band_coverage(ref, ok)


def check_closest(got, mode):
    ref, t = reference().closest, gc.closest_table()
    rows = whole_range_rows() if mode == CLOSEST_WHOLE else np.arange(t.n)
    assert_rows_equal("closest mode %d" % mode, {"d": ref.d[rows], "seg": ref.seg[rows], "xy": ref.xy[rows]},
                         {"d": got.d[rows], "seg": got.seg[rows], "xy": got.xy[rows]},
                         {"pl": t.row_pl[rows], "s0": t.row_s0[rows], "s1": t.row_s1[rows], "q": t.q[rows]})
    closest_coverage(ref, rows, ranges=mode != CLOSEST_WHOLE)


def check_broken_tables(hs, lds_on_host):
    """the input contract is checked before any item runs: -1, outputs untouched"""
    w = gc.walk_table()
    n = 4
    st, sg, xy = _sent_u(n), _sent_u(n), _sent_f((n, 2))

    def call(vtx=w.vtx, nv=w.nv, pl_off=w.pl_off, row_pl=w.row_pl[:n], row_seg=w.row_seg[:n], form=2):
        vtx, pl_off, row_pl, row_seg = (np.ascontiguousarray(a) for a in (vtx, pl_off, row_pl, row_seg))
        return hs.walk(form, _f(vtx), nv, _u(pl_off), _u(w.pl_start), _u(w.pl_end), w.npl, n, _u(row_pl), _u(row_seg),
                       _u(w.row_dir[:n].copy()), _f(w.row_f[:n].copy()), _b(w.row_bnd[:n].copy()), _u(st), _u(sg), _f(xy))

    assert call() == 0
    st[:] = gc.SENT_U32
    bad_seg = w.row_seg[:n].copy(); bad_seg[1] = w.row_size[1] - 1
    bad_off = w.pl_off.copy(); bad_off[3] = bad_off[2] + 1
    desc_off = w.pl_off.copy(); desc_off[5] = desc_off[4] - 1
    nan_vtx = w.vtx.copy(); nan_vtx[17, 1] = np.nan
    pad_inf = w.vtx.copy(); pad_inf[-1, 0] = np.inf
    bad_pl = w.row_pl[:n].copy(); bad_pl[2] = w.npl
    assert call(row_seg=bad_seg) == -1 and call(pl_off=bad_off) == -1 and call(pl_off=desc_off) == -1
    assert call(vtx=nan_vtx) == -1 and call(vtx=pad_inf) == -1 and call(row_pl=bad_pl) == -1
    assert call(nv=w.nv + 5) == -1 and call(form=99) == -1
    if lds_on_host:   # (no address_space(3) on the host)
        assert call(form=LDS_FORM) == -1
    else:             # the LDS form takes its rows grouped by polyline, ascending (polylines 0 and 1 have two vertices each)
        assert (w.row_size[:n] == 2).all() and w.pl_size[1] == 2
        assert call(form=LDS_FORM, row_pl=np.array([1, 0, 0, 0], np.uint32)) == -1
    assert (st == gc.SENT_U32).all()
    c = gc.closest_table()
    s1 = c.row_s1.copy(); s1[7] = 100000
    d, sgc, xyc = _sent_f(c.n), _sent_u(c.n), _sent_f((c.n, 2))
    rc = hs.closest(1, _f(c.vtx), c.nv, _u(c.pl_off), c.npl, _f(c.bb), len(c.bb), _u(c.bb_off), c.n, _u(c.row_pl),
                    _u(c.row_s0), _u(s1), _f(c.q), _f(d), _u(sgc), _f(xyc))
    assert rc == -1 and (sgc == gc.SENT_U32).all()
    bbo = c.bb_off.copy(); bbo[1:] += 1
    rc = hs.closest(2, _f(c.vtx), c.nv, _u(c.pl_off), c.npl, _f(c.bb), len(c.bb), _u(bbo), c.n, _u(c.row_pl),
                    _u(c.row_s0), _u(c.row_s1), _f(c.q), _f(d), _u(sgc), _f(xyc))
    assert rc == -1
    seg = gc.seg_table().rows[:8].copy(); seg[3, 2] = np.nan
    assert hs.seg(1, 8, _f(seg), _u(_sent_u(8)), _f(_sent_f((8, 2)))) == -1
