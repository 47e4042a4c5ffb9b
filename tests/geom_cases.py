"""Case tables for the geometry and walk primitives of edgegraph3d_amd/csrc/eg3d_dev_geom.h (and epiline of eg3d_dev_tri.h),
shared by the CPU half (tests/test_geom_cases.py: the oracle against the host compilation of the header) and the GPU half
(tests/test_gpu_geom_primitives.py: the same rows through the gfx950 compilation, tests/probe). Pure numpy with fixed seeds;
nothing of the product is imported (three constants are READ from the headers' text: EG3D_FOLLOW_MIN / _MAX, EG3D_BB_SEGS).

Input contract of everything in here that goes to the oracle or the GPU: coordinates finite and within +-1e7 px
(include/eg3d.h), every polyline >= 2 vertices, every start point on its segment with seg <= n - 2. The only non-finite
numbers are the NaN / infinite QUERY points of the closest-point scans, which the header documents.

  walk_table()     polylines of SIZES vertices x SHAPES x {open, loop} + a family scaled to ~1e6 px; per polyline NQ queries:
                   start on the first / last / an interior segment, at parameter 0 / 1 / inside, towards start / end / a node
                   that is neither, a distance of DISTANCES, and a line of one of the FAMILIES:
                     cross   through the neighbourhood of a vertex ahead
                     miss    every vertex >= 50 px on one side of it (the walk reaches the extreme)
                     vertex  exactly through a vertex ahead, axis-aligned or diagonal: hit parameter exactly 0 or 1, lb == 0,
                             and den == 0 on the axis-aligned segments of the staircase
                     qp      quasi-parallel to a segment ahead: cosine within +-2e-4 of 0.965 (or +-0.03), the segment's
                             first vertex 5 px +- 1e-3 (or 0..8 px) from the line
                     bound   crossing the polyline where the chord from the start point is a bound of the window +- 1e-3
                             (or +- 2): the windows are [5, 15] and [EG3D_FOLLOW_MIN, EG3D_FOLLOW_MAX]
                   unbounded and bounded.
  seg_table()      single segments x lines for seg_line_hit / seg_line_hit_guarded / seg_line_cos_gt: the partial segment and
                   one whole segment ahead of every walk row (so: the same families), zero-length segments, and segments /
                   lines whose aa * bb leaves (1e-30, 1e30) (the degenerate branch of seg_line_cos_gt), segments whose cosine
                   is within a few ulps of 0.965f (where its comparison of squares rounds differently from the division and
                   square root, so that only the band it re-evaluates keeps the decisions equal); point rows for
                   point_line_dist (sent to the oracle as zero-length segments: den == 0, the distance branch).
  cell_table()     cell sizes 4 / 10 / 30 x coordinates inside a 1600 x 1200 image, exact multiples k * cell (k <= 60),
                   +-1 / +-2 / +-16 ulp around them, the band below a multiple where ceil - v crosses 0.001 (ulp by ulp),
                   0, negatives down to -1e4, values up to 1e7; for cell_window also the image borders and map sizes that
                   put the point in the first cell, the last cell and past the last one.
  closest_table()  the six polyline kinds of test_closest_point_scan_with_box_pretest_equals_the_plain_scan; queries near,
                   far, on a vertex, equidistant between far-apart segments, NaN / infinite; ranges [s0, s1) that cut blocks
                   of EG3D_BB_SEGS, empty ranges, ranges from 0 and from 1; the block boxes by upload_block_boxes' rule.
  epiline_table()  F matrices handed in by the caller (two synthetic rigs), the same scaled by 1e+-12, a pair marked
                   invalid, a matrix whose first two rows are zero (nu == 0), points across the image.
"""
import math
import os
import re

import numpy as np

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(header, name):
    text = open(os.path.join(ROOT, "edgegraph3d_amd", "csrc", header)).read()
    m = re.search(r"#define\s+%s\s+([0-9.]+)f?\b" % name, text)
    assert m, (header, name)
    return float(m.group(1))


FOLLOW_MIN = _header_constant("eg3d_dev_follow.h", "EG3D_FOLLOW_MIN")
FOLLOW_MAX = _header_constant("eg3d_dev_follow.h", "EG3D_FOLLOW_MAX")
BB_SEGS = int(_header_constant("eg3d_dev_geom.h", "EG3D_BB_SEGS"))
WINDOWS = ((5.0, 15.0), (FOLLOW_MIN, FOLLOW_MAX))

SIZES = (2, 3, 4, 5, 6, 7, 64, 65, 66, 129, 300)
SHAPES = ("spiral", "random_walk", "staircase", "stroke")
DISTANCES = (0.5, 3.0, 10.0, 20.0, 50.0, 1e6)
FAMILIES = ("cross", "miss", "vertex", "qp", "bound")
FAM_CROSS, FAM_MISS, FAM_VERTEX, FAM_QP, FAM_BOUND = range(5)
NQ = 280
QP_COS = F32(0.965)
QP_BAND = 2e-4
QP_DIST = 5.0
NEITHER = 0xfffffff0          # a node id that is neither end of any polyline here
DIR_START, DIR_END, DIR_NEITHER = 0, 1, 2

# walk status bits (eg3d_dev_geom.h)
WALK_FOUND, WALK_EXTREME, WALK_QUASIPARALLEL, WALK_BOUND, WALK_BAD_DIR = 1, 2, 4, 8, 16

# what the outputs hold before a primitive runs: "left untouched" is visible in the result
SENT_U32 = 0xdeadbeef
SENT_F32 = np.array([0xc640e6b7], np.uint32).view(np.float32)[0]   # -12345.678
SENT_I32 = -559038737


def polyline_shape(rng, kind, n):
    """the four shapes of test_walks_with_vertex_loads_in_flight_equal_the_plain_walks"""
    if kind == "spiral":
        tt = np.linspace(0, rng.uniform(1, 12), n)
        v = np.stack([np.cos(tt) * tt * 20, np.sin(tt) * tt * 20], 1)
    elif kind == "random_walk":   # with repeated vertices (zero-length segments where two of them are neighbours)
        v = np.cumsum(rng.normal(0, 3, (n, 2)), 0)
        v[rng.integers(0, n, n // 5)] = v[0]
        if n > 4:
            v[n // 2] = v[n // 2 - 1]
    elif kind == "staircase":     # integer, axis-aligned or diagonal steps, some of length zero
        v = np.cumsum(np.stack([rng.integers(0, 3, n), rng.integers(0, 3, n)], 1), 0).astype(np.float64)
    else:                         # a nearly straight stroke
        v = np.stack([np.linspace(0, 4 * n, n), rng.normal(0, 0.5, n)], 1)
    return np.ascontiguousarray(v, np.float32)


def _line_through(px, py, ang):
    """a x + b y + c = 0 through (px, py) with direction angle ang; a, b rounded to float first"""
    a, b = F32(-math.sin(ang)), F32(math.cos(ang))
    return a, b, F32(-(float(a) * px + float(b) * py))


def _one_query(rng, v, v64, k, scale):
    """one walk row on polyline v: (seg, x, y, dir, la, lb, lc, distance, bounded, min_d, max_d, family) and the segments
    (x1 y1 x2 y2, in walking order) it contributes to the segment table"""
    n = len(v)
    fam = k % 5
    r = rng.random()
    seg = 0 if r < 0.2 else (n - 2 if r < 0.4 else int(rng.integers(0, n - 1)))
    r = rng.random()
    t = F32(0.0) if r < 0.2 else (F32(1.0) if r < 0.3 else F32(rng.random()))
    a, b = v[seg], v[seg + 1]
    px, py = F32(a[0] + F32(t * F32(b[0] - a[0]))), F32(a[1] + F32(t * F32(b[1] - a[1])))
    r = rng.random()
    d = DIR_START if r < 0.45 else (DIR_END if r < 0.9 else DIR_NEITHER)
    to_start = d == DIR_START or (d == DIR_NEITHER and rng.random() < 0.5)   # (which way the line is built for)
    ahead = list(range(seg, -1, -1)) if to_start else list(range(seg + 1, n))
    p64 = (float(px), float(py))
    bounded = bool(rng.integers(0, 2))
    win = WINDOWS[int(rng.integers(0, 2))]
    line = None
    pick = [j for j in (0, 1, 2, 3, 5, 8, 70, 200) if j < len(ahead)]
    kk = pick[int(rng.integers(0, len(pick)))]                                 # the segment ahead the row aims at
    sa = p64 if kk == 0 else tuple(v64[ahead[kk - 1]])
    sb = tuple(v64[ahead[kk]])
    if fam == FAM_BOUND:
        bounded = True
        B = (5.0, 15.0, FOLLOW_MIN, FOLLOW_MAX)[int(rng.integers(0, 4))]
        win = WINDOWS[0] if B in WINDOWS[0] else WINDOWS[1]
        target = B + (rng.uniform(-1e-3, 1e-3) if rng.random() < 0.6 else rng.uniform(-2, 2))
        dist = np.hypot(v64[ahead, 0] - p64[0], v64[ahead, 1] - p64[1])
        far = np.flatnonzero(dist >= target)
        if len(far):
            i = int(far[0])
            a0 = p64 if i == 0 else tuple(v64[ahead[i - 1]])
            b0 = tuple(v64[ahead[i]])
            ex, ey, fx, fy = b0[0] - a0[0], b0[1] - a0[1], a0[0] - p64[0], a0[1] - p64[1]
            qa, qb, qc = ex * ex + ey * ey, 2 * (ex * fx + ey * fy), fx * fx + fy * fy - target * target
            disc = qb * qb - 4 * qa * qc
            if qa > 0 and disc >= 0:
                s = min(1.0, max(0.0, (-qb + math.sqrt(disc)) / (2 * qa)))
                line = _line_through(a0[0] + s * ex, a0[1] + s * ey, math.atan2(ey, ex) + math.pi / 2 + rng.uniform(-0.3, 0.3))
                sa, sb = a0, b0
    elif fam == FAM_MISS:
        ang = rng.uniform(0, 2 * math.pi)
        ux, uy = F32(math.cos(ang)), F32(math.sin(ang))
        reach = float(np.max(v64[:, 0] * float(ux) + v64[:, 1] * float(uy)))
        line = (ux, uy, F32(-(reach + 50.0 * scale + abs(reach) * 1e-3)))
    elif fam == FAM_VERTEX:
        x, y = (px, py) if rng.random() < 0.25 else v[ahead[kk]]   # (or through the start point itself: parameter 0 at once)
        line = ((F32(1), F32(0), F32(-x)), (F32(0), F32(1), F32(-y)), (F32(1), F32(1), F32(-F32(x + y))),
                (F32(1), F32(-1), F32(-F32(x - y))))[int(rng.integers(0, 4))]
    elif fam == FAM_QP:
        ex, ey = sb[0] - sa[0], sb[1] - sa[1]
        if ex != 0 or ey != 0:
            delta = rng.uniform(-QP_BAND, QP_BAND) if rng.random() < 0.6 else rng.uniform(-0.03, 0.03)
            theta = math.acos(min(1.0, float(QP_COS) + delta)) * (1 if rng.random() < 0.5 else -1)
            # (the cosine is signed against the line's direction (1, -a/b), x > 0: a segment that walks towards -x gets
            # about -0.965 and is not quasi-parallel; both signs occur, by the polyline's shape and the walk's direction)
            ang = math.atan2(ey, ex) + theta
            off = (QP_DIST + rng.uniform(-1e-3, 1e-3)) if rng.random() < 0.6 else rng.uniform(0, 8)
            off *= 1 if rng.random() < 0.5 else -1
            line = _line_through(sa[0] - math.sin(ang) * off, sa[1] + math.cos(ang) * off, ang)
    if line is None:   # FAM_CROSS, and the fall-back of the others
        q = v64[ahead[kk]] + rng.normal(0, 1, 2) * 0.5 * scale
        line = _line_through(q[0], q[1], rng.uniform(0, math.pi))
    distance = DISTANCES[int(rng.integers(0, len(DISTANCES)))]
    row = (seg, px, py, d, line[0], line[1], line[2], F32(distance), bounded, F32(win[0]), F32(win[1]), fam)
    segs = []
    if d != DIR_NEITHER:
        e0 = v[ahead[0]]
        segs.append((px, py, e0[0], e0[1]))
        if kk > 0:
            segs.append((F32(sa[0]), F32(sa[1]), F32(sb[0]), F32(sb[1])))
        if fam == FAM_VERTEX and kk + 1 < len(ahead):   # the segment that STARTS at the vertex the line goes through
            e1 = v[ahead[kk + 1]]
            segs.append((F32(sb[0]), F32(sb[1]), e1[0], e1[1]))
    return row, segs


class WalkTable:
    """Polylines (vtx with ONE SPARE VERTEX behind the last one, pl_off, pl_start, pl_end, per polyline: size, shape, loop,
    scaled) and rows (row_pl ascending, row_seg, row_dirkind, row_dir = the node id, row_f [n][8] = x y la lb lc distance
    min_d max_d, row_bnd, row_fam)."""

    def __init__(self):
        rng = np.random.default_rng(20250)
        vt, off, start, end, meta = [], [0], [], [], []
        rows, segrows, segfam = [], [], []
        row_pl = []
        specs = [(n, s, loop, False) for n in SIZES for s in SHAPES for loop in (False, True)]
        specs += [(n, s, False, True) for n in SIZES for s in ("spiral", "stroke")]
        for (n, shape, loop, scaled) in specs:
            v = polyline_shape(rng, shape, n)
            scale = 1.0
            if scaled:   # about 1e6 px, inside the +-1e7 of the contract
                scale = 1e6 / max(1.0, float(np.abs(v).max()))
                v = np.ascontiguousarray(v.astype(np.float64) * scale, np.float32)
            p = len(start)
            vt.append(v)
            off.append(off[-1] + n)
            start.append(7 if loop else 1)
            end.append(7 if loop else 2)
            meta.append((n, shape, loop, scaled))
            v64 = v.astype(np.float64)
            for k in range(NQ):
                row, segs = _one_query(rng, v, v64, k, scale)
                rows.append(row)
                row_pl.append(p)
                for s in segs:
                    segrows.append(s + (row[4], row[5], row[6]))
                    segfam.append(row[11])
        vtx = np.concatenate(vt + [np.zeros((1, 2), np.float32)])   # the spare vertex
        self.vtx = np.ascontiguousarray(vtx, np.float32)
        self.nv = len(self.vtx) - 1
        self.pl_off = np.array(off, np.uint32)
        self.pl_start = np.array(start, np.uint32)
        self.pl_end = np.array(end, np.uint32)
        self.npl = len(start)
        self.pl_size = np.array([m[0] for m in meta], np.int32)
        self.pl_shape = [m[1] for m in meta]
        self.pl_loop = np.array([m[2] for m in meta], bool)
        self.pl_scaled = np.array([m[3] for m in meta], bool)
        self.n = len(rows)
        self.row_pl = np.array(row_pl, np.uint32)
        self.row_seg = np.array([r[0] for r in rows], np.uint32)
        self.row_dirkind = np.array([r[3] for r in rows], np.int32)
        node = np.where(self.row_dirkind == DIR_START, self.pl_start[self.row_pl],
                        np.where(self.row_dirkind == DIR_END, self.pl_end[self.row_pl], NEITHER))
        self.row_dir = np.ascontiguousarray(node, np.uint32)
        self.row_f = np.ascontiguousarray([[r[1], r[2], r[4], r[5], r[6], r[7], r[9], r[10]] for r in rows], np.float32)
        self.row_bnd = np.array([r[8] for r in rows], np.uint8)
        self.row_fam = np.array([r[11] for r in rows], np.int32)
        self.row_size = self.pl_size[self.row_pl]
        self.seg_rows = np.ascontiguousarray(segrows, np.float32)    # [m][7], for seg_table()
        self.seg_fam = np.array(segfam, np.int32)
        assert np.isfinite(self.vtx).all() and np.abs(self.vtx).max() <= 1e7 and np.isfinite(self.row_f).all()
        assert (self.row_seg <= self.row_size - 2).all() and (np.diff(self.row_pl.astype(np.int64)) >= 0).all()


_CACHE = {}


def _cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def walk_table():
    return _cached("walk", WalkTable)


class SegTable:
    """rows [n][8] = x1 y1 x2 y2 la lb lc thr (thr = 0.965f); fam = the family (FAMILIES index, 5 zero-length, 6 degenerate
    magnitudes, 7 the cosine within a few ulps of the threshold); points = the rows of point_line_dist, [m][8] with x2 y2 = x1 y1."""

    def __init__(self):
        w = walk_table()
        rng = np.random.default_rng(20251)
        base = w.seg_rows
        # zero-length segments on lines at every distance
        m = 600
        zp = rng.uniform(-800, 800, (m, 2))
        zp[:100] = np.round(zp[:100])
        ang = rng.uniform(0, math.pi, m)
        off = np.where(rng.random(m) < 0.5, 5.0 + rng.uniform(-1e-3, 1e-3, m), rng.uniform(0, 12, m))
        za, zb = np.float32(-np.sin(ang)), np.float32(np.cos(ang))
        zc = -(za.astype(np.float64) * (zp[:, 0] - np.sin(ang) * off) + zb.astype(np.float64) * (zp[:, 1] + np.cos(ang) * off))
        zero = np.stack([zp[:, 0], zp[:, 1], zp[:, 0], zp[:, 1], za, zb, zc], 1).astype(np.float32)
        zero[:, 2:4] = zero[:, 0:2]
        zero[:50, 4:6] = [1.0, 0.0]   # lb == 0
        zero[50:100, 4:6] = [0.0, 1.0]
        # aa * bb outside (1e-30, 1e30): tiny segments, steep lines (bb = 1 + (a/b)^2 huge), long segments on steep lines,
        # bb = +inf; with the segment along and against the line's direction, and the products just inside the range too
        deg = []
        for i in range(600):
            kind = i % 6
            th = rng.uniform(0, 2 * math.pi)
            x1, y1 = (rng.uniform(-100, 100, 2) if kind else (0.0, 0.0))
            if kind == 0:      # aa ~ 1e-32 .. 1e-30 around the lower edge (segments next to the origin: the difference is exact)
                L = 10.0 ** rng.uniform(-17, -14.5)
                x1, y1 = 0.0, 0.0
                la, lb = math.sin(th + rng.normal(0, 0.3)), -math.cos(th + rng.normal(0, 0.3))
            elif kind == 1:    # bb ~ 1e28 .. 1e34
                L = rng.uniform(0.5, 30)
                la, lb = 1.0, 10.0 ** rng.uniform(-17, -14) * (1 if rng.random() < 0.5 else -1)
                th = (math.pi / 2 if rng.random() < 0.5 else -math.pi / 2) + rng.normal(0, 0.2)
            elif kind == 2:    # long segments (aa ~ 1e13) on steep lines (bb ~ 1e16 .. 1e18)
                L = rng.uniform(1e6, 5e6)
                la, lb = 1.0, 10.0 ** rng.uniform(-9, -8) * (1 if rng.random() < 0.5 else -1)
                th = (math.pi / 2 if rng.random() < 0.5 else -math.pi / 2) + rng.normal(0, 0.2)
            elif kind == 3:    # bb = +inf
                L = rng.uniform(0.5, 30)
                la, lb = 1.0, 10.0 ** rng.uniform(-30, -20)
            elif kind == 4:    # aa * bb = 0 by underflow: a segment of a few denormal-sized steps
                L = 1e-30
                x1, y1 = 0.0, 0.0
                la, lb = math.sin(th), -math.cos(th)
            else:              # the knife edge at ordinary magnitudes, for contrast
                L = rng.uniform(0.5, 30)
                t2 = th + math.acos(0.965 + rng.uniform(-QP_BAND, QP_BAND))
                la, lb = -math.sin(t2), math.cos(t2)
            x2, y2 = x1 + L * math.cos(th), y1 + L * math.sin(th)
            lc = -(la * x1 + lb * y1) + rng.uniform(-6, 6)
            deg.append((x1, y1, x2, y2, la, lb, lc))
        deg = np.array(deg, np.float32)
        # the knife edge ULP BY ULP: segments from the origin (exact differences) whose cosine against the line is 0.965f in
        # exact arithmetic for a real ay, with ay's nine nearest floats: the computed cosine lands on the threshold and a few
        # ulps to either side of it, where the comparison of squares and the plain expression can round differently
        m = 700
        la, lb = np.float32(rng.uniform(-1, 1, m)), np.float32(rng.uniform(0.05, 1, m) * rng.choice([-1, 1], m))
        by = (-la / lb).astype(np.float64)
        thr = float(QP_COS)
        L = rng.uniform(0.5, 60, m)
        phi = np.arctan(by) + np.arccos(thr) * rng.choice([-1, 1], m)
        ax = np.float32(L * np.cos(phi)).astype(np.float64)
        g = lambda ay: (ax + ay * by) / np.sqrt((ax * ax + ay * ay) * (1 + by * by)) - thr
        lo, hi = L * np.sin(phi) - 0.02 * L, L * np.sin(phi) + 0.02 * L
        ok = (g(lo) * g(hi) < 0) & (np.abs(ax) > 1e-3)
        for _ in range(70):
            mid = 0.5 * (lo + hi)
            left = g(lo) * g(mid) <= 0
            hi, lo = np.where(left, mid, hi), np.where(left, lo, mid)
        ay0 = np.float32(0.5 * (lo + hi))
        ulp = []
        for k in range(-4, 5):
            ay = _ulps(ay0, k)
            ulp.append(np.stack([np.zeros(m), np.zeros(m), ax, ay, la, lb, np.float32(rng.uniform(-6, 6, m))], 1)[ok])
        ulp = np.concatenate(ulp).astype(np.float32)
        rows = np.concatenate([base, zero, deg, ulp])
        self.fam = np.concatenate([w.seg_fam, np.full(len(zero), 5, np.int32), np.full(len(deg), 6, np.int32),
                                   np.full(len(ulp), 7, np.int32)])
        self.rows = np.ascontiguousarray(np.concatenate([rows, np.full((len(rows), 1), QP_COS, np.float32)], 1), np.float32)
        self.n = len(self.rows)
        # point_line_dist: the start points of the walk rows and the zero-length rows, each against its line
        pts = np.concatenate([np.stack([w.row_f[:, 0], w.row_f[:, 1], w.row_f[:, 0], w.row_f[:, 1], w.row_f[:, 2], w.row_f[:, 3],
                                        w.row_f[:, 4]], 1)[::3], zero])
        self.points = np.ascontiguousarray(np.concatenate([pts, np.full((len(pts), 1), QP_COS, np.float32)], 1), np.float32)
        assert np.isfinite(self.rows).all() and np.abs(self.rows[:, :4]).max() <= 1e7 and np.isfinite(self.points).all()


def seg_table():
    return _cached("seg", SegTable)


CELLS = (4.0, 10.0, 30.0)
IMG_W, IMG_H = 1600, 1200


def _ulps(x, k):
    """the float k ulps above (k > 0) or below x"""
    x = np.asarray(x, np.float32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def cell_values(cell):
    """(values, tag): tag 0 uniform, 1 exact multiple, 2 ulps around a multiple, 3 the 0.001 band (runs of 17 consecutive
    floats), 4 zero / negative, 5 large"""
    rng = np.random.default_rng(int(cell) + 20252)
    ks = np.arange(0, 61, dtype=np.float64)
    mult = (ks * cell).astype(np.float32)
    vals, tags = [rng.uniform(0, 1600, 1500).astype(np.float32)], [np.zeros(1500, np.int32)]
    vals.append(mult); tags.append(np.full(len(mult), 1, np.int32))
    for u in (1, 2, 16, -1, -2, -16):
        vals.append(_ulps(mult, u)); tags.append(np.full(len(mult), 2, np.int32))
    # cell_round(v) takes the ceiling when (double)(ceil(v) - v) < 0.001: v = x / cell crosses that at x ~ (k - 0.001) * cell
    centre = ((ks[1:] - 0.001) * cell).astype(np.float32)
    for u in range(-8, 9):
        vals.append(_ulps(centre, u)); tags.append(np.full(len(centre), 3, np.int32))
    neg = np.array([0.0, -0.0, -1e-3, -0.5, -1.0, -3.999, -4.0, -10.0, -29.9995, -30.0, -123.4, -1000.0, -9999.5, -1e4], np.float32)
    vals.append(neg); tags.append(np.full(len(neg), 4, np.int32))
    big = np.array([1599.9995, 1600.0, 1e5, 123456.7, 1e6, 9999999.0, 1e7], np.float32)
    vals.append(big); tags.append(np.full(len(big), 5, np.int32))
    return np.concatenate(vals), np.concatenate(tags)


class CellTable:
    """cell_of rows: rows [n][3] = cell x y with tag_x / tag_y; cell_window rows: wrows [m][3] and wdims [m][4] = img_w img_h
    map_w map_h, wkind 0 the map of the image, 1 the point's cell is the last one, 2 it lies past the last one, 3 the first"""

    def __init__(self):
        rng = np.random.default_rng(20253)
        rows, tx, ty = [], [], []
        wrows, wdims, wkind = [], [], []
        for cell in CELLS:
            v, t = cell_values(cell)
            perm = rng.permutation(len(v))
            for (a, ta, b, tb) in ((v, t, v[perm], t[perm]), (v[perm], t[perm], v, t)):
                rows.append(np.stack([np.full(len(a), cell, np.float32), a, b], 1))
                tx.append(ta); ty.append(tb)
            # windows: points of every tag inside the image (and a little outside), the borders, each with several maps
            inside = v[(v > -2) & (v < 1700)]
            xs = np.concatenate([inside, _ulps([0.0, IMG_W], 1), _ulps([0.0, IMG_W], -1), np.array([0, IMG_W, -1, IMG_W + 1], np.float32)])
            ys = np.concatenate([inside[inside < 1300], _ulps([0.0, IMG_H], 1), _ulps([0.0, IMG_H], -1),
                                 np.array([0, IMG_H, -1, IMG_H + 1], np.float32)])
            m = max(len(xs), len(ys))
            x = np.concatenate([xs, rng.uniform(0, IMG_W, m - len(xs)).astype(np.float32)])[rng.permutation(m)]
            y = np.concatenate([ys, rng.uniform(0, IMG_H, m - len(ys)).astype(np.float32)])[rng.permutation(m)]
            mw, mh = int(math.ceil(IMG_W / cell)), int(math.ceil(IMG_H / cell))
            cx = np.floor(x.astype(np.float64) / cell).astype(np.int64)
            cy = np.floor(y.astype(np.float64) / cell).astype(np.int64)
            for kind in range(4):
                if kind == 0:
                    w_, h_ = np.full(m, mw), np.full(m, mh)
                elif kind == 1:
                    w_, h_ = np.maximum(1, cx + 1), np.maximum(1, cy + 1)
                elif kind == 2:
                    w_, h_ = np.maximum(1, cx), np.maximum(1, cy - 1)
                else:
                    w_, h_ = np.full(m, mw), np.full(m, mh)
                xx, yy = x, y
                if kind == 3:   # the first cell
                    xx = (x.astype(np.float64) % cell).astype(np.float32)
                    yy = (y.astype(np.float64) % cell).astype(np.float32)
                wrows.append(np.stack([np.full(m, cell, np.float32), xx, yy], 1))
                wdims.append(np.stack([np.full(m, IMG_W), np.full(m, IMG_H), w_, h_], 1))
                wkind.append(np.full(m, kind, np.int32))
        self.rows = np.ascontiguousarray(np.concatenate(rows), np.float32)
        self.tag_x, self.tag_y = np.concatenate(tx), np.concatenate(ty)
        self.n = len(self.rows)
        self.dims = np.ascontiguousarray(np.tile(np.array([IMG_W, IMG_H, 1, 1], np.int32), (self.n, 1)))   # (unused by cell_of)
        self.wrows = np.ascontiguousarray(np.concatenate(wrows), np.float32)
        self.wdims = np.ascontiguousarray(np.concatenate(wdims), np.int32)
        self.wkind = np.concatenate(wkind)
        self.m = len(self.wrows)
        assert np.isfinite(self.rows).all() and np.abs(self.rows).max() <= 1e7 and (self.wdims >= 1).all()


def cell_table():
    return _cached("cell", CellTable)


def block_boxes(v):
    """upload_block_boxes (eg3d_api.hip): per block of BB_SEGS segments the box of its BB_SEGS + 1 vertices"""
    nseg = len(v) - 1
    out = []
    for s0 in range(0, nseg, BB_SEGS):
        s1 = min(nseg, s0 + BB_SEGS)
        q = v[s0:s1 + 1]
        out.append([q[:, 0].min(), q[:, 1].min(), q[:, 0].max(), q[:, 1].max()])
    return np.array(out, np.float32).reshape(-1, 4)


CLOSEST_KINDS = ("curve", "random_walk", "two_passes", "integer_grid", "staircase", "uniform")
CLOSEST_SIZES = (2, 3, 9, 17, 40, 130, 257)


def closest_polyline(rng, kind, n):
    """the six kinds of test_closest_point_scan_with_box_pretest_equals_the_plain_scan"""
    if kind == "curve":
        tt = np.linspace(0, rng.uniform(1, 12), n)
        v = np.stack([np.cos(tt) * tt * 20, np.sin(tt) * tt * 20], 1)
    elif kind == "random_walk":
        v = np.cumsum(rng.normal(0, 3, (n, 2)), 0)
        v[rng.integers(0, n, n // 5)] = v[0]
    elif kind == "two_passes":   # two identical passes over the same stroke: exact ties between far-apart segments
        h = np.cumsum(rng.normal(0, 2, ((n + 1) // 2, 2)), 0)
        v = np.concatenate([h, h[::-1]])[:n]
    elif kind == "integer_grid":
        v = rng.integers(-30, 30, (n, 2)).astype(np.float64)
    elif kind == "staircase":
        v = np.cumsum(np.stack([rng.integers(0, 3, n), rng.integers(0, 3, n)], 1), 0).astype(np.float64)
    else:
        v = rng.uniform(-500, 500, (n, 2))
    return v


class ClosestTable:
    """polylines (vtx with one spare vertex, pl_off, boxes bb / bb_off) and rows (row_pl, row_s0, row_s1, q [n][2], row_kind:
    0 near, 1 far, 2 on a vertex, 3 equidistant, 4 NaN / infinite)"""

    def __init__(self):
        rng = np.random.default_rng(20254)
        vt, off, bb, bbo, kinds = [], [0], [], [0], []
        rp, s0s, s1s, qs, qk = [], [], [], [], []
        for ki, kind in enumerate(CLOSEST_KINDS):
            for si, n in enumerate(CLOSEST_SIZES):
                extent = (None, 1e4, 5e6)[(si + ki) % 3] if kind in ("curve", "uniform") else None   # inside the +-1e7 px accepted
                v = closest_polyline(rng, kind, n)
                if extent:
                    v = v * (extent / max(1.0, float(np.abs(v).max())))
                v = np.ascontiguousarray(v, np.float32)
                p = len(kinds)
                kinds.append(kind)
                vt.append(v)
                off.append(off[-1] + n)
                b = block_boxes(v)
                bb.append(b)
                bbo.append(bbo[-1] + len(b))
                nseg = n - 1
                ext = float(np.abs(v).max()) + 1.0
                near = v[rng.integers(0, n, 24)] + (rng.normal(0, 4, (24, 2)) * max(1.0, ext / 1000.0)).astype(np.float32)
                far = (rng.uniform(-2, 2, (8, 2)) * ext).astype(np.float32)
                onv = v[rng.integers(0, n, 8)]
                i, j = rng.integers(0, nseg, 8), rng.integers(0, nseg, 8)
                mid = ((v[i].astype(np.float64) + v[i + 1] + v[j] + v[j + 1]) / 4).astype(np.float32)   # between two segments
                if kind == "two_passes":   # on the stroke itself: both passes at distance exactly 0 / exactly equal
                    mid = ((v[i].astype(np.float64) + v[i + 1]) / 2).astype(np.float32)
                odd = np.array([[np.nan, 0], [0, np.nan], [np.inf, 1], [-np.inf, -np.inf], [1e30, -1e30], [0, 0]], np.float32)
                q = np.concatenate([near, far, onv, mid, odd])
                k = np.concatenate([np.zeros(24), np.ones(8), np.full(8, 2), np.full(8, 3), np.full(6, 4)]).astype(np.int32)
                cut = [int(c) for c in sorted(rng.integers(0, nseg + 1, 2))]
                ranges = [(0, nseg), (0, 0), (min(1, nseg), nseg), (0, cut[1]), (cut[0], cut[1]), (cut[1], cut[1]),
                          (min(nseg, BB_SEGS - 1), min(nseg, 2 * BB_SEGS + 1))]
                for (a, e) in ranges:
                    rp.append(np.full(len(q), p)); s0s.append(np.full(len(q), a)); s1s.append(np.full(len(q), e))
                    qs.append(q); qk.append(k)
        self.vtx = np.ascontiguousarray(np.concatenate(vt + [np.zeros((1, 2), np.float32)]), np.float32)
        self.nv = len(self.vtx) - 1
        self.pl_off = np.array(off, np.uint32)
        self.npl = len(kinds)
        self.pl_kind = kinds
        self.bb = np.ascontiguousarray(np.concatenate(bb), np.float32)
        self.bb_off = np.array(bbo, np.uint32)
        self.row_pl = np.concatenate(rp).astype(np.uint32)
        self.row_s0 = np.concatenate(s0s).astype(np.uint32)
        self.row_s1 = np.concatenate(s1s).astype(np.uint32)
        self.q = np.ascontiguousarray(np.concatenate(qs), np.float32)
        self.row_kind = np.concatenate(qk)
        self.n = len(self.q)
        assert np.isfinite(self.vtx).all() and np.abs(self.vtx).max() <= 1e7


def closest_table():
    return _cached("closest", ClosestTable)


class EpilineTable:
    """F [n][9], valid [n], xy [n][2], kind [n]: 0 a rig's matrix, 1 scaled by 1e12, 2 by 1e-12, 3 marked invalid, 4 first two
    rows zero (nu == 0: the line stays unnormalised)"""

    def __init__(self, F_list):
        rng = np.random.default_rng(20255)
        mats = np.concatenate([np.asarray(F, np.float64).reshape(-1, 9) for F in F_list])
        mats = mats[np.abs(mats).sum(1) > 0]
        assert len(mats) >= 4 and np.isfinite(mats).all()
        grid = np.stack(np.meshgrid(np.linspace(0, IMG_W, 9), np.linspace(0, IMG_H, 7)), -1).reshape(-1, 2)
        pts = np.concatenate([grid, rng.uniform(0, [IMG_W, IMG_H], (17, 2))]).astype(np.float32)
        F, valid, xy, kind = [], [], [], []
        for k in range(5):
            for m in mats:
                M = m.copy()
                if k == 1:
                    M = M * 1e12
                elif k == 2:
                    M = M * 1e-12
                elif k == 4:
                    M[:6] = 0.0
                F.append(np.tile(M, (len(pts), 1)))
                valid.append(np.full(len(pts), 0 if k == 3 else 1, np.uint8))
                xy.append(pts)
                kind.append(np.full(len(pts), k, np.int32))
        self.F = np.ascontiguousarray(np.concatenate(F), np.float64)
        self.valid = np.concatenate(valid)
        self.xy = np.ascontiguousarray(np.concatenate(xy), np.float32)
        self.kind = np.concatenate(kind)
        self.n = len(self.xy)


def epiline_table(F_list):
    return EpilineTable(F_list)
