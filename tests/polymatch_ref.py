"""Test reference of pipeline 2's polyline matcher: a restatement of the reference's
polyline_matching_closeness_to_refpoints (matching/polyline_matching/polyline_matcher.cpp:75-168) in Python.

It is built ONLY on primitives the CPU oracle exports (orc_cell_from_coords, orc_next_by_distance, orc_batch_mindist,
orc_get_grid for the pin test) and imports nothing from the product libraries. Everything above those primitives — the
map (polyLine_2d_map.cpp:40-58, polyline_graph_2d.cpp:555-577,819-835), the window rule and the distance filter
(polyLine_2d_map_search.cpp:46-77,122-137), the rule per reference point (polyline_matcher.cpp:106-148), the node numbering
and the stack-based component walk (graph_adjacency_set_undirected_no_type.cpp:44-69) — is written out as the reference
has it. A scene is the dict of numpy arrays host.Synth.scene_np() returns; seeds are (trk_off, trk_view, trk_xy).
"""
import ctypes as C

import numpy as np

from oracle import binding as ob

FIND_WITHIN_DIST = 10.0
F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny   # std::numeric_limits<float>::min(): the smallest positive NORMAL float


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def cell_from_coords(cell, x, y):
    """get_2dmap_cell_from_coords with both boundary flags: (col, row, on_boundary_row, on_boundary_col)."""
    col, row, br, bc = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    ob.lib().orc_cell_from_coords(float(cell), float(x), float(y), C.byref(col), C.byref(row), C.byref(br), C.byref(bc))
    return col.value, row.value, bool(br.value), bool(bc.value)


def polyline_samples(vtx, start, end, step):
    """split_equal_size_intervals(start, step): the start point, then next_pl_point_by_distance towards the other end until
    the extreme is reached."""
    L = ob.lib()
    v = np.ascontiguousarray(vtx, np.float32)
    out = [(float(v[0, 0]), float(v[0, 1]))]
    seg, x, y = 0, v[0, 0], v[0, 1]
    oseg, oxy = C.c_uint32(), np.zeros(2, np.float32)
    while True:
        reached = L.orc_next_by_distance(_f32p(v), len(v), int(start), int(end), seg, float(x), float(y), int(end),
                                         float(step), C.byref(oseg), _f32p(oxy))
        seg, x, y = oseg.value, oxy[0], oxy[1]
        out.append((float(x), float(y)))
        if reached:
            return out


def build_map(scene, view, cell):
    """PolyLine2DMap(plg, img_sz, cell): (ncols, nrows, off, ids), cell index = row * ncols + col, ids ascending per cell.
    A sample whose cell lies outside the map is dropped (the reference indexes out of bounds there)."""
    cell = F32(cell)
    ncols = int(np.ceil(F32(scene["width"]) / cell))
    nrows = int(np.ceil(F32(scene["height"]) / cell))
    step = F32(float(cell) / (1.414 + 0.1))   # cell_dim / PL_CELL_SPLIT_RATIO: float / double, passed as float
    lists = [[] for _ in range(ncols * nrows)]
    g0, g1 = int(scene["view_pl_off"][view]), int(scene["view_pl_off"][view + 1])
    for g in range(g0, g1):
        if not scene["pl_valid"][g]:
            continue
        a, b = int(scene["pl_vtx_off"][g]), int(scene["pl_vtx_off"][g + 1])
        cells = set()
        for (x, y) in polyline_samples(scene["vtx_xy"][a:b], scene["pl_start"][g], scene["pl_end"][g], step):
            col, row, br, bc = cell_from_coords(cell, x, y)
            if not (br or bc) and 0 <= col < ncols and 0 <= row < nrows:
                cells.add((col, row))
        for (col, row) in cells:
            lists[row * ncols + col].append(g - g0)
    off = np.zeros(ncols * nrows + 1, np.uint32)
    off[1:] = np.cumsum([len(l) for l in lists])
    ids = np.array([i for l in lists for i in l], np.uint32)
    return ncols, nrows, off, ids


def compute_distancesq(vtx, x, y):
    """polyline::compute_distancesq: the first smallest minimum_distancesq over the segments."""
    v = np.ascontiguousarray(vtx, np.float32)
    n = len(v) - 1
    q = np.empty((n, 6), np.float32)
    q[:, 0], q[:, 1] = x, y
    q[:, 2:4], q[:, 4:6] = v[:-1], v[1:]
    out = np.zeros((n, 3), np.float32)
    ob.lib().orc_batch_mindist(n, _f32p(q), _f32p(out))
    best = out[0, 0]
    for i in range(1, n):
        if out[i, 0] < best:
            best = out[i, 0]
    return F32(best)


def window_rule(width, height, ncols, nrows, x, y, cc):
    """The cells find_polylines_within_search_dist_with_reprojections visits around (x, y) (polyLine_2d_map_search.cpp:46-77):
    cc = cell_from_coords(cell, x, y) = (col, row, on_boundary_row, on_boundary_col). None for a point on or outside the
    image border, else (col0, col1, row0, row1), inclusive. (The one statement of the rule: search() below and the
    cell_window rows of tests/test_geom_cases.py both use it.)"""
    x, y = F32(x), F32(y)
    if x <= 0 or x >= width or y <= 0 or y >= height:
        return None
    col, row, b_row, b_col = cc() if callable(cc) else cc   # (a callable is evaluated for points inside the image only)
    col = ncols - 1 if (col < 0 or col >= ncols) else col   # (the reference compares as unsigned)
    row = nrows - 1 if (row < 0 or row >= nrows) else row
    i0 = -1 if row > 0 else 0
    i1 = 0 if b_row else (1 if row < nrows - 1 else 0)
    j0 = -1 if col > 0 else 0
    j1 = 0 if b_col else (1 if col < ncols - 1 else 0)
    return col + j0, col + j1, row + i0, row + i1


def search(scene, view, grid, x, y):
    """find_polylines_within_search_dist_with_reprojections at (x, y) of `view`: [(polyline id, distance as float)]."""
    ncols, nrows, off, ids = grid
    x, y = F32(x), F32(y)
    w = window_rule(scene["width"], scene["height"], ncols, nrows, x, y, lambda: cell_from_coords(FIND_WITHIN_DIST, x, y))
    if w is None:
        return []
    c0, c1, r0, r1 = w
    cand = set()
    for r in range(r0, r1 + 1):
        for cl in range(c0, c1 + 1):
            c = r * ncols + cl
            cand.update(int(p) for p in ids[off[c]:off[c + 1]])
    res = []
    g0 = int(scene["view_pl_off"][view])
    for pl in sorted(cand):
        a, b = int(scene["pl_vtx_off"][g0 + pl]), int(scene["pl_vtx_off"][g0 + pl + 1])
        d2 = compute_distancesq(scene["vtx_xy"][a:b], x, y)
        if d2 <= F32(100.0):
            res.append((pl, F32(np.sqrt(d2))))
    return res


def observation(trk_view, trk_xy, t0, t1, view):
    """get_2d_coordinates_of_point_on_image: the observation of the track in `view` — the LAST entry that names the view
    (the convention the whole project follows for a track that lists a view twice)."""
    x = y = F32(0)
    for e in range(t0, t1):
        if trk_view[e] == view:
            x, y = trk_xy[e]
    return x, y


def refpoint_rule(views, results):
    """polyline_matcher.cpp:106-148 on one point: views = the track's view ids, results = per entry the search result.
    Returns the ascending list of distinct (view, polyline) if the point is accepted, None otherwise."""
    maxpl = 0
    for r in results:
        maxpl = len(r) if maxpl < len(r) else maxpl
    if maxpl != 1:
        return None
    pairs = set()
    min_dist, max_dist = F32(FLT_MAX), F32(FLT_MIN)
    for i, r in enumerate(results):
        if len(r) == 0:
            continue
        pl, d = r[0]
        d = F32(d)
        min_dist = min_dist if min_dist <= d else d
        max_dist = max_dist if max_dist >= d else d
        pairs.add((int(views[i]), int(pl)))
    if float(len(pairs)) < len(views) * 0.7:       # double
        return None
    with np.errstate(over="ignore", under="ignore"):
        if min_dist < F32(max_dist / F32(3)):      # float
            return None
        if max_dist > F32(min_dist * F32(3)):
            return None
    if len(pairs) < 2:
        return None
    return sorted(pairs)


def components_stack_walk(n_nodes, adjacency):
    """GraphAdjacencySetUndirectedNoType::get_components: components in the order of their smallest node id, each in the
    order the stack visits it. adjacency: list of sets (iterated ascending, as std::set)."""
    visited = [False] * n_nodes
    res = []
    for s in range(n_nodes):
        if visited[s]:
            continue
        cur, stack = [], [s]
        visited[s] = True
        while stack:
            n = stack.pop()
            cur.append(n)
            for m in sorted(adjacency[n]):
                if not visited[m]:
                    visited[m] = True
                    stack.append(m)
        res.append(cur)
    return res


def match_graph(accepted_pairs):
    """The match graph of the accepted points, in order: accepted_pairs = [(point id, sorted [(view, polyline)])].
    Returns (node list [(view, polyline)] by first appearance, adjacency sets)."""
    node_of, nodes, adj = {}, [], []
    for _, pairs in accepted_pairs:
        ids = []
        for p in pairs:
            if p not in node_of:
                node_of[p] = len(nodes)
                nodes.append(p)
                adj.append(set())
            ids.append(node_of[p])
        for i in range(len(ids)):
            for j in range(i + 1, len(ids)):
                adj[ids[i]].add(ids[j])
                adj[ids[j]].add(ids[i])
    return nodes, adj


def sets_from_components(nodes, comps, n_views):
    """vector<vector<set<ulong>>> -> the CSR of eg3d_polyline_sets: rows set * n_views + view, ids ascending."""
    row_off, pl_ids = [0], []
    for comp in comps:
        per_view = [set() for _ in range(n_views)]
        for n in comp:
            per_view[nodes[n][0]].add(nodes[n][1])
        for v in range(n_views):
            pl_ids.extend(sorted(per_view[v]))
            row_off.append(len(pl_ids))
    return np.array(row_off, np.uint32), np.array(pl_ids, np.uint32)


def match_from_results(n_views, points):
    """points: [(point id, track view ids, per-entry results)] ascending. Returns the reference's result."""
    accepted = []
    for pid, views, results in points:
        pairs = refpoint_rule(views, results)
        if pairs is not None:
            accepted.append((pid, pairs))
    nodes, adj = match_graph(accepted)
    comps = components_stack_walk(len(nodes), adj)
    row_off, pl_ids = sets_from_components(nodes, comps, n_views)
    return {"refpoints": np.array([p for p, _ in accepted], np.uint32), "n_sets": len(comps), "row_off": row_off,
            "pl_ids": pl_ids}


class Matcher:
    """The 10 px maps of a scene (built once) and the matcher on seed ranges of it."""

    def __init__(self, scene):
        self.scene = scene
        self.grids = [build_map(scene, v, FIND_WITHIN_DIST) for v in range(int(scene["n_views"]))]

    def entry_results(self, seeds, begin, end):
        trk_off, trk_view, trk_xy = seeds
        pts = []
        for r in range(begin, end):
            t0, t1 = int(trk_off[r]), int(trk_off[r + 1])
            res = []
            for e in range(t0, t1):
                v = int(trk_view[e])
                x, y = observation(trk_view, trk_xy, t0, t1, v)
                res.append(search(self.scene, v, self.grids[v], x, y))
            pts.append((r, [int(v) for v in trk_view[t0:t1]], res))
        return pts

    def match(self, seeds, begin, end):
        return match_from_results(int(self.scene["n_views"]), self.entry_results(seeds, begin, end))


def reject_reason(views, results):
    """Which test of the rule rejects the point (None: accepted): 'maxpl', 'share', 'min', 'max', 'two'."""
    if max([len(r) for r in results] + [0]) != 1:
        return "maxpl"
    d = [F32(r[0][1]) for r in results if r]
    pairs = {(int(views[i]), int(r[0][0])) for i, r in enumerate(results) if r}
    mn, mx = min([F32(FLT_MAX)] + d), max([F32(FLT_MIN)] + d)
    if float(len(pairs)) < len(views) * 0.7:
        return "share"
    with np.errstate(over="ignore", under="ignore"):
        if mn < F32(mx / F32(3)):
            return "min"
        if mx > F32(mn * F32(3)):
            return "max"
    return "two" if len(pairs) < 2 else None
