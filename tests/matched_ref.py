"""Independent restatement of what the pipelines 1-2 extractor does when the caller's PLGMatchesManager holds intervals
(eg3d_match_polyline_sets_matched / eg3d_polyline_set_candidates / eg3d_host_is_matched).

Written from the reference's text — PLGMatchesManager::is_matched (plg_matches_manager.cpp:54-85), polyline::
interval_contains_plp (polyline_graph_2d.cpp:269-293), the walk of find_new_3d_points_from_compatible_polylines_
expandallviews_parallel (polyline_matching.cpp:153-201) and find_epipolar_correspondences (:45-73) — in Python, with the
reference's control flow (an iterator that steps backwards, not a binary search) and built ONLY on probes the CPU oracle
exports: orc_next_by_distance, orc_epiline, orc_intersect_segment_line (and Oracle.replay_matches for the intervals, in the
tests). No product code is used.

Arithmetic: segment indices are the reference's `ulong` (M1: `start.segment_index - 1` wraps modulo 2^64); coordinates are
float32 and every product / difference of is_ordered_2dlinepoints is rounded to float32 as the reference's `float`
expressions are (-ffp-contract=off: no fused multiply-add).

Two things the reference leaves open are fixed here as the product documents them (csrc/eg3d_matched_core.h):
  M4   every interval of the row starts after the point: the reference decrements begin() — "not matched";
  walk a jump to the end of a containing interval that does not land strictly further along the polyline than the sample it
       came from (the reference then loops for ever): NoProgress is raised — the intervals do not belong to the scene."""
import ctypes as C

import numpy as np

U64 = 1 << 64
SPLIT = 20.0
f32 = np.float32


class NoProgress(ValueError):
    pass


# ---- the rule -------------------------------------------------------------------------------------------------------------
def ordered(a, b, c):
    """is_ordered_2dlinepoints (geometric_utilities.cpp:1375-1377) on float32 pairs"""
    ax, ay, bx, by, cx, cy = f32(a[0]), f32(a[1]), f32(b[0]), f32(b[1]), f32(c[0]), f32(c[1])
    return bool(f32(bx - ax) * f32(cx - bx) > 0 or f32(by - ay) * f32(cy - by) > 0 or (ax == bx and ay == by) or
                (bx == cx and by == cy))


def _eq(a, b):
    return f32(a[0]) == f32(b[0]) and f32(a[1]) == f32(b[1])


class Interval:
    __slots__ = ("sseg", "sxy", "eseg", "exy")

    def __init__(self, sseg, sxy, eseg, exy):
        self.sseg, self.eseg = int(sseg), int(eseg)
        self.sxy = (f32(sxy[0]), f32(sxy[1]))
        self.exy = (f32(exy[0]), f32(exy[1]))


def interval_contains_plp(iv, v, seg, xy):
    """polyline::interval_contains_plp; v = the polyline's vertices [n, 2]"""
    seg = int(seg)
    if seg < (iv.sseg - 1) % U64 or seg > (iv.eseg + 1) % U64:  # M1
        return False
    if seg > iv.sseg and seg < iv.sseg:  # M2 (:272, as written)
        return True
    if seg == iv.sseg:
        if ordered(v[iv.sseg], iv.sxy, xy):
            if iv.eseg == iv.sseg:
                return ordered(iv.sxy, xy, iv.exy)
            return True
        return False
    if seg == iv.eseg:
        return ordered(v[iv.eseg], xy, iv.exy)
    if seg == iv.eseg + 1 and _eq(v[seg], xy) and _eq(iv.exy, v[seg]):
        return True
    if seg == (iv.sseg - 1) % U64 and _eq(v[seg + 1], xy) and _eq(iv.sxy, v[seg + 1]):
        return True
    return False


def is_matched(row, v, seg, xy):
    """PLGMatchesManager::is_matched on one (view, polyline)'s intervals (a list of Interval, start segments strictly
    ascending: the reference's std::set ordered by start.segment_index). Returns the index of the containing interval or -1."""
    n = len(row) if row else 0
    if n == 0:
        return -1
    seg = int(seg)
    it = 0  # lower_bound(interval starting at plp)
    while it < n and row[it].sseg < seg:
        it += 1
    if it == n or row[it].sseg > seg:
        if it == 0:
            return -1  # M4
        it -= 1
    reached_begin, found = False, -1
    while not reached_begin and row[it].sseg == seg:  # for(; it->start == seg && !reached_begin; it--)
        if it == 0:
            reached_begin = True
        if interval_contains_plp(row[it], v, seg, xy):
            found = it
            break
        it -= 1
    if found < 0 and not reached_begin and row[it].eseg <= seg:
        if interval_contains_plp(row[it], v, seg, xy):
            found = it
    return found


def dist2(a, b):
    """squared distance as the reference computes it (geometric_utilities.cpp:555-557): float differences, double squares"""
    dx, dy = float(f32(a[0]) - f32(b[0])), float(f32(a[1]) - f32(b[1]))
    return f32(dx * dx + dy * dy)


def progresses(v, last, nxt):
    """nxt = (seg, xy) lies strictly further along the polyline than last: (segment, squared distance from its first vertex)"""
    if nxt[0] != last[0]:
        return nxt[0] > last[0]
    return bool(dist2(v[nxt[0]], nxt[1]) > dist2(v[last[0]], last[1]))


# ---- scene plumbing (numpy only) ------------------------------------------------------------------------------------------
class Scene:
    """A scene dict (host.Synth.scene_np() / sets_cases.Case.scene) + the oracle's probe library."""

    def __init__(self, scene, oracle_lib):
        self.sc, self.L = scene, oracle_lib
        self.V = int(scene["n_views"])
        self.vpo = np.asarray(scene["view_pl_off"], np.int64)
        self.pvo = np.asarray(scene["pl_vtx_off"], np.int64)

    def gid(self, view, pl):
        return int(self.vpo[view]) + int(pl)

    def vertices(self, g):
        if not self.sc["pl_valid"][g]:
            return np.zeros((0, 2), np.float32)
        return np.ascontiguousarray(self.sc["vtx_xy"][self.pvo[g]:self.pvo[g + 1]], np.float32)

    def next_by_distance(self, g, v, seg, xy):
        """polyline::next_pl_point_by_distance(plp, pl.end, 20): (reached_end, seg, xy)"""
        oseg, oxy = C.c_uint32(), np.zeros(2, np.float32)
        end = int(self.sc["pl_end"][g])
        r = self.L.orc_next_by_distance(v.ctypes.data_as(C.POINTER(C.c_float)), len(v), int(self.sc["pl_start"][g]), end,
                                        int(seg), float(xy[0]), float(xy[1]), end, SPLIT, C.byref(oseg),
                                        oxy.ctypes.data_as(C.POINTER(C.c_float)))
        return bool(r), int(oseg.value), (f32(oxy[0]), f32(oxy[1]))

    def epiline(self, frm, to, xy):
        if not self.sc["F_valid"][frm][to]:
            return None
        F = np.ascontiguousarray(self.sc["F"][frm][to], np.float64).reshape(9)
        line = np.zeros(3, np.float32)
        ok = self.L.orc_epiline(F.ctypes.data_as(C.POINTER(C.c_double)), float(xy[0]), float(xy[1]),
                                line.ctypes.data_as(C.POINTER(C.c_float)))
        return line if ok else None

    def intersect_line(self, v, line):
        """polyline::intersect_line: [(segment, xy)] in segment order, the segment (v[i], v[i-1]) tagged i - 1"""
        out = []
        inter = np.zeros(2, np.float32)
        par, ovl = C.c_int(), C.c_int()
        lp, ip = line.ctypes.data_as(C.POINTER(C.c_float)), inter.ctypes.data_as(C.POINTER(C.c_float))
        for i in range(1, len(v)):
            if self.L.orc_intersect_segment_line(float(v[i][0]), float(v[i][1]), float(v[i - 1][0]), float(v[i - 1][1]), lp, ip,
                                                 C.byref(par), C.byref(ovl)):
                out.append((i - 1, (f32(inter[0]), f32(inter[1]))))
        return out


def rows_of(graph, n_scene_polylines=None):
    """matched_polyline_intervals as {global polyline: [Interval]} from a graph dict (Oracle.replay_matches)"""
    if graph is None:
        return {}
    off = np.asarray(graph["iv_off"], np.uint64)
    rows = {}
    for g in range(len(off) - 1):
        a, b = int(off[g]), int(off[g + 1])
        if b > a:
            rows[g] = [Interval(graph["iv_start_seg"][k], graph["iv_start_xy"][k], graph["iv_end_seg"][k], graph["iv_end_xy"][k])
                       for k in range(a, b)]
    return rows


# ---- the walk and stage A -------------------------------------------------------------------------------------------------
def walk(S, view, pl, row):
    """The samples of one polyline that become tasks, and the number skipped (polyline_matching.cpp:168-190)."""
    g = S.gid(view, pl)
    v = S.vertices(g)
    tasks, skipped = [], 0
    if len(v) < 2:
        return tasks, skipped
    reached, seg, xy = S.next_by_distance(g, v, 0, (v[0][0], v[0][1]))
    last = None
    while not reached:
        if row:
            if last is not None and not progresses(v, last, (seg, xy)):
                raise NoProgress("view %d polyline %d: the walk does not advance at segment %d" % (view, pl, seg))
            last = (seg, xy)
        k = is_matched(row, v, seg, xy)
        if k < 0:
            tasks.append((seg, xy))
            reached, seg, xy = S.next_by_distance(g, v, seg, xy)
        else:  # jump to interval end
            skipped += 1
            reached, seg, xy = S.next_by_distance(g, v, row[k].eseg, row[k].exy)
    return tasks, skipped


def jump_ok(S, view, pl, row, k, seg, xy):
    """What the host probe refuses: the walk from the end of interval k does not get past the point it contains. A closed
    polyline (start node == end node) yields no sample, so nothing jumps on it."""
    g = S.gid(view, pl)
    if int(S.sc["pl_start"][g]) == int(S.sc["pl_end"][g]):
        return True
    v = S.vertices(g)
    reached, nseg, nxy = S.next_by_distance(g, v, row[k].eseg, row[k].exy)
    return reached or progresses(v, (int(seg), xy), (nseg, nxy))


def stage_a(S, n_sets, row_off, pl_ids, graph=None, begin=0, end=None):
    """Stage A of the extractor on sets [begin, end) in the layout of Context.polyline_set_candidates."""
    end = n_sets if end is None else end
    V = S.V
    rows = rows_of(graph)
    t_view, t_pl, t_seg, t_xy, list_off, h_pl, h_seg, h_xy, t_set = [], [], [], [], [0], [], [], [], []
    skipped = filtered = 0
    for s in range(begin, end):
        ids = [[int(p) for p in pl_ids[row_off[s * V + v]:row_off[s * V + v + 1]]] for v in range(V)]
        for sv in range(V):
            for pl in ids[sv]:
                tasks, sk = walk(S, sv, pl, rows.get(S.gid(sv, pl)))
                skipped += sk
                for seg, xy in tasks:
                    t_view.append(sv), t_pl.append(pl), t_seg.append(seg), t_xy.append(xy), t_set.append(s)
                    for ov in range(V):
                        if ov == sv:
                            h_pl.append(pl), h_seg.append(seg), h_xy.append(xy)
                        else:
                            line = S.epiline(sv, ov, xy)
                            if line is not None:
                                for opl in ids[ov]:
                                    g = S.gid(ov, opl)
                                    v = S.vertices(g)
                                    row = rows.get(g)
                                    for hseg, hxy in S.intersect_line(v, line):
                                        if row and is_matched(row, v, hseg, hxy) >= 0:
                                            filtered += 1
                                            continue
                                        h_pl.append(opl), h_seg.append(hseg), h_xy.append(hxy)
                        list_off.append(len(h_pl))
    nt, nh = len(t_view), len(h_pl)
    return {"n_tasks": nt, "task_view": np.asarray(t_view, np.int32), "task_pl": np.asarray(t_pl, np.uint32),
            "task_seg": np.asarray(t_seg, np.uint32), "task_xy": np.asarray(t_xy, np.float32).reshape(nt, 2),
            "list_off": np.asarray(list_off, np.uint64), "hit_pl": np.asarray(h_pl, np.uint32),
            "hit_seg": np.asarray(h_seg, np.uint32), "hit_xy": np.asarray(h_xy, np.float32).reshape(nh, 2),
            "n_samples_skipped": skipped, "n_hits_filtered": filtered, "task_set": np.asarray(t_set, np.int64)}


def same_candidates(ref, got):
    """None, or what differs first (bit patterns of the coordinates compared)."""
    for k in ("n_tasks", "n_samples_skipped", "n_hits_filtered"):
        if int(ref[k]) != int(got[k]):
            return "%s: %d != %d" % (k, ref[k], got[k])
    for k in ("task_view", "task_pl", "task_seg", "list_off", "hit_pl", "hit_seg"):
        if not np.array_equal(np.asarray(ref[k], np.int64), np.asarray(got[k], np.int64)):
            return k
    for k in ("task_xy", "hit_xy"):
        a = np.ascontiguousarray(ref[k], np.float32).view(np.uint32)
        b = np.ascontiguousarray(got[k], np.float32).view(np.uint32)
        if a.shape != b.shape or not np.array_equal(a, b):
            return k
    return None
