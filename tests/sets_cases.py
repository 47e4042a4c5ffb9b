"""Irregular "potentially compatible polylines" sets for the pipelines 1-2 extractor (eg3d_match_polyline_sets), shared by
its GPU parity test (tests/test_gpu_polyline_sets.py) and the CPU checks of the extractor's sampling
(tests/test_sets_sampling.py).

host.Synth.polyline_sets() gives one set per synthetic 3-D curve: valid polylines of >= 2 vertices, each in exactly one
set, most views present, dozens of samples per set. The reference's sets come from the similarity-graph / Louvain matcher
(polyline_matching.cpp:153-208 takes them as vector<set<ulong>>) and look different: small, overlapping, many views
missing, short polylines. Each family below is built to reach one branch of the extractor that curve-sized sets never do:

  tiny        hundreds of sets of 1-3 pieces of 20-60 px chord: one wavefront of 64 samples spans many sets (k_n1_hits)
  one_view    sets whose rows are empty in every view but one (k_n1_samples' find_owner over runs of empty rows)
  sparse      a 12-view rig, sets present in 1-3 views, empty sets at the ends of sub-ranges
  overlap     a polyline in several sets, sets that are supersets of others, a set repeated
  degenerate  ids of invalid polylines (stray vertices left in the input), of 0- and 1-vertex polylines and of loops
  exact       a rectified rig (cameras that differ by an x translation only, epipolar lines y = const) with integer,
              axis-aligned polylines: samples at exactly 20*k px of chord and epipolar lines through shared vertices
  bound_lo    V < 64: runs of sets of exactly max_items = 16384 polyline ids and one more, one set above the bound
  bound_hi    V = 64: the same at max_items = 2048

Every row is strictly ascending (the reference's set<ulong>). All scenes are generated with seeded RNGs."""
import numpy as np

from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import host

SPLIT = 20.0  # SPLIT_INTERVAL_DISTANCE (polyline_matching.hpp:51)
WAVE = 64
MAX_ITEMS_LO, MAX_ITEMS_HI = 16384, 2048  # eg3d_match_polyline_sets: the unit bound for V < 64 / V >= 64


class Case:
    """One scene + one list of sets. sets[i] = {view: sorted polyline ids}; csr() gives (n_sets, row_off, pl_ids).
    subranges: [set_b, set_e) ranges to compare with the slice of the whole call. units: for the bound families,
    (set_b, set_e, number of units eg3d_match_polyline_sets must cut the range into)."""

    def __init__(self, name, scene, sets, subranges=(), units=(), meta=None):
        self.name = name
        self.scene = scene  # dict in the layout of host.Synth.scene_np()
        self.V = int(scene["n_views"])
        self.sets = sets
        self.subranges = list(subranges)
        self.units = list(units)
        self.meta = dict(meta or {})
        self._arrays = None

    @property
    def n_sets(self):
        return len(self.sets)

    def scene_arrays(self):
        if self._arrays is None:
            self._arrays = host.SceneArrays(self.scene)
        return self._arrays

    def csr(self):
        return to_csr(self.sets, self.V)

    def n_pl(self, v):
        vpo = self.scene["view_pl_off"]
        return int(vpo[v + 1] - vpo[v])

    def polyline(self, v, p):
        """vertices (float32 [n, 2]) of view-local polyline p of view v, as the product sees them (none if invalid)"""
        g = int(self.scene["view_pl_off"][v]) + p
        if not self.scene["pl_valid"][g]:
            return np.zeros((0, 2), np.float32)
        pvo = self.scene["pl_vtx_off"]
        return self.scene["vtx_xy"][pvo[g]:pvo[g + 1]]

    def kind(self, v, p):
        """'short' (< 2 vertices in the input, valid or not, or a valid chord under 20 px), 'invalid' (the others with
        pl_valid == 0), 'loop' (start node == end node) or 'plain'"""
        g = int(self.scene["view_pl_off"][v]) + p
        pvo = self.scene["pl_vtx_off"]
        xy = self.scene["vtx_xy"][pvo[g]:pvo[g + 1]]
        if len(xy) < 2:
            return "short"
        if not self.scene["pl_valid"][g]:
            return "invalid"
        if np.linalg.norm(xy.astype(np.float64) - xy[0], axis=1).max() < SPLIT:
            return "short"
        if self.scene["pl_start"][g] == self.scene["pl_end"][g]:
            return "loop"
        return "plain"


def to_csr(sets, V):
    row_off, ids = [0], []
    for s in sets:
        for v in range(V):
            row = sorted(s.get(v, ()))
            assert all(b > a for a, b in zip(row, row[1:])), "a row must be strictly ascending"
            ids.extend(row)
            row_off.append(len(ids))
    return len(sets), np.asarray(row_off, np.uint32), np.asarray(ids, np.uint32)


def rows_strictly_ascending(n_sets, row_off, pl_ids, V):
    for r in range(n_sets * V):
        row = np.asarray(pl_ids[row_off[r]:row_off[r + 1]], np.int64)
        if len(row) > 1 and not (np.diff(row) > 0).all():
            return False
    return True


def _synth(cfg_index, **over):
    cfg = host.default_config(cfg_index)
    for k, v in over.items():
        setattr(cfg, k, v)
    return host.Synth(cfg)


def _curves(s):
    """view-local polyline ids of every (curve, view): valid polylines of >= 2 vertices, as Synth.polyline_sets()"""
    sc = s.scene_np()
    V, vpo = sc["n_views"], sc["view_pl_off"]
    NP = int(vpo[-1])
    curve = D.as_np(host.lib().eg3d_synth_polyline_curve(s._h), NP, np.uint32)
    n_curves = int(host.lib().eg3d_synth_n_curves(s._h))
    nvtx = np.diff(sc["pl_vtx_off"])
    out = [[[] for _ in range(V)] for _ in range(n_curves)]
    for v in range(V):
        for p in range(int(vpo[v + 1] - vpo[v])):
            g = int(vpo[v]) + p
            if sc["pl_valid"][g] and nvtx[g] >= 2 and curve[g] < n_curves:
                out[int(curve[g])][v].append(p)
    return sc, out


def _with_polylines(sc, per_view):
    """sc with the polylines of every view replaced: per_view[v] = list of (vertices [n,2], start, end, valid)"""
    V = int(sc["n_views"])
    vpo, pvo, vtx, st, en, va = [0], [0], [], [], [], []
    for v in range(V):
        for (xy, a, b, ok) in per_view[v]:
            xy = np.asarray(xy, np.float32).reshape(-1, 2)
            vtx.extend(xy.tolist())
            pvo.append(len(vtx))
            st.append(a)
            en.append(b)
            va.append(1 if ok else 0)
        vpo.append(len(st))
    out = dict(sc)
    out.update(view_pl_off=np.asarray(vpo, np.uint32), pl_vtx_off=np.asarray(pvo, np.uint32),
               vtx_xy=np.asarray(vtx, np.float32).reshape(-1, 2),
               pl_start=np.asarray(st, np.uint32), pl_end=np.asarray(en, np.uint32), pl_valid=np.asarray(va, np.uint8))
    return out


def _polylines_of(sc):
    V = int(sc["n_views"])
    vpo, pvo = sc["view_pl_off"], sc["pl_vtx_off"]
    per_view = []
    for v in range(V):
        cur = []
        for g in range(int(vpo[v]), int(vpo[v + 1])):
            cur.append((sc["vtx_xy"][pvo[g]:pvo[g + 1]].copy(), int(sc["pl_start"][g]), int(sc["pl_end"][g]),
                        bool(sc["pl_valid"][g])))
        per_view.append(cur)
    return per_view


# ---------------------------------------------------------------------------------------------------------- families --
def _first_sample(xy):
    """the point 20 px of chord from the start of a polyline (float64), None if it has none"""
    p0 = xy[0].astype(np.float64)
    for i in range(1, len(xy)):
        d1 = np.linalg.norm(xy[i].astype(np.float64) - p0)
        if d1 >= SPLIT:
            d0 = np.linalg.norm(xy[i - 1].astype(np.float64) - p0)
            return xy[i - 1] + (xy[i].astype(np.float64) - xy[i - 1]) * ((SPLIT - d0) / (d1 - d0))
    return None


def _crosses(xy, line):
    s = xy.astype(np.float64) @ line[:2] + line[2]
    return bool((np.sign(s[1:]) != np.sign(s[:-1])).any())


def tiny(seed=101):
    """The config-1 scene with every polyline cut into pieces of 20-60 px of chord (consecutive vertices, own nodes),
    and 420 sets of 1-3 pieces of one curve: a piece, plus pieces of other views that its first sample's epipolar line
    crosses (so that sets of three views emit chains). Most pieces hold one sample: a wave of 64 samples spans dozens
    of sets."""
    rng = np.random.default_rng(seed)
    s = host.Synth(1)
    sc, _ = _curves(s)
    V, vpo, pvo, vtx = int(sc["n_views"]), sc["view_pl_off"], sc["pl_vtx_off"], sc["vtx_xy"]
    NP = int(vpo[-1])
    curve = D.as_np(host.lib().eg3d_synth_polyline_curve(s._h), NP, np.uint32)
    per_view, pieces = [], {}  # pieces[(curve, view)] = view-local piece ids
    node = 0
    for v in range(V):
        cur = []
        for g in range(int(vpo[v]), int(vpo[v + 1])):
            xy = vtx[pvo[g]:pvo[g + 1]]
            if not sc["pl_valid"][g] or len(xy) < 2:
                continue
            i = 0
            while i < len(xy) - 1:
                target = rng.uniform(21.0, 39.0) if rng.random() < 0.85 else rng.uniform(40.0, 59.0)
                j = i + 1
                while j < len(xy) - 1 and np.linalg.norm(xy[j].astype(np.float64) - xy[i]) < target:
                    j += 1
                chord = float(np.linalg.norm(xy[j].astype(np.float64) - xy[i]))
                if 20.0 <= chord <= 60.0:
                    pieces.setdefault((int(curve[g]), v), []).append(len(cur))
                    cur.append((xy[i:j + 1].copy(), node, node + 1, True))
                    node += 2
                i = j
        per_view.append(cur)
    scene = _with_polylines(sc, per_view)
    F = scene["F"]
    flat = sorted((c, v, p) for (c, v), ps in pieces.items() for p in ps)
    sets = []
    for _ in range(420):
        c, v, p = flat[int(rng.integers(len(flat)))]
        k = int(rng.choice([1, 1, 1, 1, 2, 2, 3]))
        st = {v: [p]}
        x = _first_sample(per_view[v][p][0])
        if x is not None and k > 1:
            for w in rng.permutation(V):
                w = int(w)
                if w == v or (c, w) not in pieces or len(st) >= k:
                    continue
                line = F[v, w].reshape(3, 3) @ np.array([x[0], x[1], 1.0])
                hit = [q for q in pieces[(c, w)] if _crosses(per_view[w][q][0], line)]
                if hit:
                    st[w] = [int(rng.choice(hit))]
        sets.append(st)
    n = len(sets)
    return Case("tiny", scene, sets, subranges=[(0, n), (1, 2), (17, 83), (200, 200), (n - 64, n)])


def one_view(seed=102):
    """Curve sets of config 1 cut to one view (each view in turn), between complete curve sets."""
    rng = np.random.default_rng(seed)
    s = host.Synth(1)
    sc, cur = _curves(s)
    V = int(sc["n_views"])
    sets = []
    for c in range(len(cur)):
        if c % 3 == 0:
            sets.append({v: list(cur[c][v]) for v in range(V) if cur[c][v]})
        for v in range(V):
            if cur[c][v] and rng.random() < 0.5:
                ids = list(cur[c][v])
                keep = sorted(rng.choice(ids, size=int(rng.integers(1, len(ids) + 1)), replace=False).tolist())
                sets.append({v: keep})
    n = len(sets)
    return Case("one_view", sc, sets, subranges=[(0, n), (1, 4), (n // 2, n // 2 + 7), (n - 1, n)])


def sparse(seed=103):
    """A 12-view rig; sets present in 1-3 views (long runs of empty rows), empty sets at the start, at the end and in
    the middle; sub-ranges that begin or end on an empty set."""
    rng = np.random.default_rng(seed)
    s = _synth(1, n_views=12, n_curves=10, n_seeds=40, max_track=12, rng_seed=0x5A5E)
    sc, cur = _curves(s)
    V = int(sc["n_views"])
    sets = [{}, {}]
    for c in range(len(cur)):
        have = [v for v in range(V) if cur[c][v]]
        for _ in range(3):
            views = sorted(rng.choice(have, size=min(len(have), int(rng.integers(1, 4))), replace=False).tolist())
            sets.append({v: list(cur[c][v]) for v in views})
        if c % 3 == 1:
            sets.append({})
    sets += [{}, {}]
    n = len(sets)
    empty = [i for i in range(n) if not sets[i]]
    sub = [(0, n), (0, 1), (0, 5), (empty[2], empty[3] + 1), (empty[2] + 1, empty[3]), (empty[3], empty[3]),
           (n - 6, n), (n - 2, n)]
    return Case("sparse", sc, sets, subranges=sub)


def overlap(seed=104):
    """Config-1 curve sets, their pairwise unions (supersets), random subsets, and exact repeats: every polyline is
    in several sets, so the same polyline is sampled once per occurrence, each time under its own key[0]."""
    rng = np.random.default_rng(seed)
    s = host.Synth(1)
    sc, cur = _curves(s)
    V = int(sc["n_views"])
    base = [{v: list(cur[c][v]) for v in range(V) if cur[c][v]} for c in range(len(cur))]
    sets = []
    for c in range(len(base)):
        sets.append(base[c])
        sub = {v: sorted(rng.choice(ids, size=max(1, len(ids) // 2), replace=False).tolist())
               for v, ids in base[c].items() if rng.random() < 0.7}
        sets.append(sub)
        d = (c + 1) % len(base)
        sets.append({v: sorted(set(base[c].get(v, [])) | set(base[d].get(v, []))) for v in range(V)
                     if base[c].get(v) or base[d].get(v)})
        if c % 4 == 0:
            sets.append(base[c])
    n = len(sets)
    return Case("overlap", sc, sets, subranges=[(0, n), (2, 9), (n - 5, n)])


def degenerate(seed=105):
    """Config 1 with polylines made invalid (all, one or none of their vertices left in the input), cut to one segment
    shorter than 20 px, straightened to their two end vertices (valid, sampled), and turned into loops (end node := start node, the last vertex moved onto the first); curve sets
    that keep those ids, and one set of each kind alone. (A VALID polyline of fewer than 2 vertices is not used: every
    polyline of the reference's graph runs between two nodes, and its get_start_plp() would read past an empty one.)"""
    rng = np.random.default_rng(seed)
    s = host.Synth(1)
    sc, cur = _curves(s)
    V = int(sc["n_views"])
    per_view = _polylines_of(sc)
    kinds = {}
    for c in range(len(cur)):
        for v in range(V):
            for p in cur[c][v]:
                r = rng.random()
                xy, a, b, ok = per_view[v][p]
                if r < 0.12:
                    per_view[v][p] = (xy, a, b, False)               # invalid, stray vertices left (Q8)
                    kinds[(v, p)] = "invalid"
                elif r < 0.18:
                    per_view[v][p] = (xy[:1], a, b, False)           # invalid, one stray vertex
                    kinds[(v, p)] = "short"
                elif r < 0.22:
                    per_view[v][p] = (xy[:0], a, b, False)           # invalidated as the reference does: no vertex
                    kinds[(v, p)] = "short"
                elif r < 0.28:
                    d = xy[1].astype(np.float64) - xy[0]
                    end = xy[0] + d * (rng.uniform(4.0, 19.0) / max(np.linalg.norm(d), 1e-3))
                    per_view[v][p] = (np.float32([xy[0], end]), a, b, True)   # valid, one segment under 20 px
                    kinds[(v, p)] = "short"
                elif r < 0.38 and len(xy) > 2:
                    per_view[v][p] = (np.float32([xy[0], xy[-1]]), a, b, True)   # valid, straightened to 2 vertices
                    kinds[(v, p)] = "two"
                elif r < 0.48:
                    xy = xy.copy()
                    xy[-1] = xy[0]
                    per_view[v][p] = (xy, a, a, True)                # loop: start node == end node
                    kinds[(v, p)] = "loop"
    scene = _with_polylines(sc, per_view)
    sets = [{v: list(cur[c][v]) for v in range(V) if cur[c][v]} for c in range(len(cur))]
    # and sets made of degenerate ids only
    for kind in ("invalid", "short", "loop"):
        st = {}
        for (v, p), k in sorted(kinds.items()):
            if k == kind:
                st.setdefault(v, []).append(p)
        sets.append(st)
    n = len(sets)
    return Case("degenerate", scene, sets, subranges=[(0, n), (3, 6), (n - 3, n)])


def rectified_scene(V=4, d=20, width=1600, height=1200, f=1000.0):
    """Cameras K [I | -C] with centres on the x axis: a point at depth Z seen in view k lies d = f*B/Z px to the left of
    its position in view k-1, on the same row. F[i][j] = [e1]x = [[0,0,0],[0,0,-1],[0,1,0]] (any pair): the epipolar line
    of (x, y) is 0*x' - y' + y = 0, exact in float."""
    cx, cy = width / 2.0, height / 2.0
    Z = 10.0
    B = d * Z / f
    P = np.zeros((V, 4, 4), np.float32)
    for k in range(V):
        P[k, 0] = [f, 0.0, cx, -f * k * B]
        P[k, 1] = [0.0, f, cy, 0.0]
        P[k, 2] = [0.0, 0.0, 1.0, 0.0]
    F = np.zeros((V, V, 9), np.float64)
    for i in range(V):
        for j in range(V):
            F[i, j] = [0, 0, 0, 0, 0, -1, 0, 1, 0]
    Fv = np.ones((V, V), np.uint8) - np.eye(V, dtype=np.uint8)
    return {"n_views": V, "width": width, "height": height, "cam_P": P.reshape(V, 16), "F": F, "F_valid": Fv}, Z


def exact(seed=106):
    """The rectified rig with curves on the plane Z = 10: integer, axis-aligned (and 3-4-5) vertices, the same in every
    view up to an integer shift of 20 px per view. Steps of 5, 10 and 20 px put vertices at exactly 20*k px of chord from
    the previous sample; every epipolar line (y = const) of a sample on a vertex goes through vertices of the other
    views, where the two adjacent segments both report t in [0, 1] (Q10)."""
    rng = np.random.default_rng(seed)
    rig, _ = rectified_scene()
    V = rig["n_views"]
    shapes = []
    for c in range(12):
        x0, y0 = 300 + 90 * (c % 6), 200 + 380 * (c // 6)
        step = [5, 10, 20][c % 3]
        pts = [(x0, y0)]
        n = int(rng.integers(6, 14))
        for i in range(n):
            x, y = pts[-1]
            kind = (c + i) % 5
            if kind == 3:
                pts.append((x + 16, y + 12))      # 3-4-5: a chord of 20 across a corner
            elif kind == 4:
                pts.append((x - 12, y + 16))
            else:
                pts.append((x, y + step))         # vertical: the epipolar lines (y = const) cross it
        shapes.append(np.asarray(pts, np.float32))
    per_view = []
    node = 0
    for k in range(V):
        cur = []
        for xy in shapes:
            cur.append((xy - np.float32([20 * k, 0]), node, node + 1, True))
            node += 2
        per_view.append(cur)
    scene = _with_polylines(dict(rig), per_view)
    n_c = len(shapes)
    sets = [{v: [c] for v in range(V)} for c in range(n_c)]
    sets.append({v: list(range(n_c)) for v in range(V)})                    # every curve in one set
    sets.append({0: [0, 1, 2], 1: [0, 1, 2], 2: [1, 2]})
    n = len(sets)
    return Case("exact", scene, sets, subranges=[(0, n), (2, 5), (n - 2, n)])


def _bound(name, V, max_items, seed):
    """Synth curves + padding: per view, max_items // V + 2 invalidated polylines, half of them with a stray vertex left
    (no sample, no segment, in no grid, but an id that counts against the unit bound). Sets: A and B sum to exactly max_items ids, A and B1 to max_items + 1, L alone holds
    more than max_items; each also holds one polyline of one curve in each of four views, so every unit emits a chain."""
    rng = np.random.default_rng(seed)
    if V < 64:
        s = host.Synth(1)
    else:
        s = _synth(1, n_views=V, n_curves=6, n_seeds=20, max_track=V, rng_seed=seed)
    sc, cur = _curves(s)
    per_view = _polylines_of(sc)
    pad0 = [len(per_view[v]) for v in range(V)]
    n_pad = max_items // V + 2
    node = 1 << 20
    for v in range(V):
        for i in range(n_pad):
            xy = np.float32([[rng.uniform(50, sc["width"] - 50), rng.uniform(50, sc["height"] - 50)]])[:i % 2]
            per_view[v].append((xy, node, node + 1, False))
            node += 2
    scene = _with_polylines(sc, per_view)
    good = [c for c in range(len(cur)) if sum(1 for v in range(V) if cur[c][v]) >= 3]

    def curve_set(c, n_items):
        st = {v: list(cur[c][v][:1]) for v in [v for v in range(V) if cur[c][v]][:4]}  # a few samples: cheap chains
        have = sum(len(x) for x in st.values())
        need = n_items - have
        assert 0 <= need <= V * n_pad
        v = 0
        while need > 0:
            take = min(need, n_pad)
            st[v] = sorted(st.get(v, []) + list(range(pad0[v], pad0[v] + take)))
            need -= take
            v += 1
        return st

    a = max_items // 2 - 37
    A = curve_set(good[0], a)
    B = curve_set(good[1], max_items - a)
    B1 = curve_set(good[1], max_items - a + 1)
    L = curve_set(good[2], max_items + 1 + V)
    sets = [A, B, A, B1, L, A, L]
    # (range, units): [A, B] = max_items exactly -> one unit; [A, B1] = max_items + 1 -> two; [L] alone -> one;
    # [B1, L] and [A, L] -> two (a set above the bound is never joined to another); [A, B, A] -> two
    units = [(0, 2, 1), (2, 4, 2), (4, 5, 1), (3, 5, 2), (5, 7, 2), (0, 3, 2)]
    sub = [(0, 7), (0, 2), (2, 4), (4, 5)]
    return Case(name, scene, sets, subranges=sub, units=units, meta={"max_items": max_items})


def bound_lo(seed=107):
    return _bound("bound_lo", 6, MAX_ITEMS_LO, seed)


def bound_hi(seed=108):
    return _bound("bound_hi", 64, MAX_ITEMS_HI, seed)


FAMILIES = {"tiny": tiny, "one_view": one_view, "sparse": sparse, "overlap": overlap, "degenerate": degenerate,
            "exact": exact, "bound_lo": bound_lo, "bound_hi": bound_hi}


# ---------------------------------------------------------------------------------------------------------- coverage --
def sets_per_wave(sample_counts):
    """Numbers of distinct sets in each wavefront of 64 consecutive samples (one call = one unit: k_n1_hits serves the
    samples of a batch 64 to a wave, in sample order). sample_counts[i] = samples of set i."""
    owner = np.repeat(np.arange(len(sample_counts)), np.asarray(sample_counts, np.int64))
    return [len(np.unique(owner[w:w + WAVE])) for w in range(0, len(owner), WAVE)]


def units_expected(row_off, V, b, e, max_items):
    """Reference restatement of eg3d_match_polyline_sets' cut on ONE lane: runs of whole sets of <= max_items ids, a set
    above the bound alone."""
    items = lambda i, j: int(row_off[j * V]) - int(row_off[i * V])
    n, s0 = 0, b
    while s0 < e:
        s1 = s0 + 1
        while s1 < e and items(s0, s1 + 1) <= max_items:
            s1 += 1
        n += 1
        s0 = s1
    return n
