"""ctypes mirrors of the POD structs the headers of include/ define, listed in MIRRORS (plumbing only)."""
import ctypes as C

import numpy as np

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
i32p = C.POINTER(C.c_int32)
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)


class Scene(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("cam_P", f32p), ("F", f64p), ("F_valid", u8p), ("view_pl_off", u32p),
                ("pl_vtx_off", u32p), ("vtx_xy", f32p), ("pl_start", u32p), ("pl_end", u32p),
                ("pl_valid", u8p)]


class Seeds(C.Structure):
    _fields_ = [("n_seeds", C.c_uint32), ("trk_off", u32p), ("trk_view", i32p), ("trk_xy", f32p)]


class PolylineSets(C.Structure):
    _fields_ = [("n_sets", C.c_uint32), ("row_off", u32p), ("pl_ids", u32p)]


class DevicePolylineSets(C.Structure):
    """eg3d_device_polyline_sets (include/eg3d_sets_device.h): a view into buffers of the context that produced it."""
    _fields_ = [("struct_size", C.c_uint32), ("n_sets", C.c_uint32), ("n_views", C.c_int32), ("device", C.c_int32),
                ("n_ids", C.c_uint64), ("row_off", C.c_void_p), ("pl_ids", C.c_void_p)]


class ItemsCall(C.Structure):
    """eg3d_items_call: the item range of one eg3d_match_polyline_items call and the samples before it."""
    _fields_ = [("struct_size", C.c_uint32), ("item_begin", C.c_uint32), ("item_end", C.c_uint32), ("sample_base", C.c_uint32)]


class SetsDeviceStats(C.Structure):
    """eg3d_sets_device_stats: struct_size is set to the size of this mirror by its user before the call."""
    _fields_ = [("struct_size", C.c_uint32), ("n_nodes", C.c_uint32), ("n_named", C.c_uint32), ("n_sets", C.c_uint32),
                ("n_ids", C.c_uint64), ("ms_device", C.c_float), ("ms_upload", C.c_float)]


class TriStats(C.Structure):
    """eg3d_tri_stats (include/eg3d_triangulate.h): struct_size is set to the size of this mirror by its user before the call."""
    _fields_ = [("struct_size", C.c_uint32), ("n_batches", C.c_uint32), ("n_tracks", C.c_uint64), ("n_valid", C.c_uint64),
                ("n_short", C.c_uint64), ("n_degenerate", C.c_uint64), ("ms_kernel", C.c_float), ("ms_stage", C.c_float),
                ("ms_copy", C.c_float)]


class ColourStats(C.Structure):
    """eg3d_colour_stats (include/eg3d_colour.h): struct_size is set to the size of this mirror by its user before the call."""
    _fields_ = [("struct_size", C.c_uint32), ("n_images", C.c_uint32), ("n_points", C.c_uint64), ("n_coloured", C.c_uint64),
                ("n_empty", C.c_uint64), ("n_obs_sampled", C.c_uint64), ("ms_sample", C.c_float), ("ms_mix", C.c_float),
                ("ms_copy", C.c_float)]


class TransformStats(C.Structure):
    """eg3d_transform_stats (include/eg3d_transform.h): struct_size is set to the size of this mirror by its user before the call."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_points", C.c_uint64), ("n_transformed", C.c_uint64),
                ("n_nonfinite", C.c_uint64), ("ms_kernel", C.c_float), ("ms_copy", C.c_float)]


class SimilarityStats(C.Structure):
    """eg3d_similarity_stats (include/eg3d_host_transform.h): struct_size is set to the size of this mirror by its user."""
    _fields_ = [("struct_size", C.c_uint32), ("n_used", C.c_uint32), ("scale", C.c_double), ("singular", C.c_double * 3),
                ("src_var", C.c_double), ("reflection", C.c_uint32), ("rank_deficient", C.c_uint32)]


class EdgeChains(C.Structure):
    """eg3d_edge_chain_set (include/eg3d/host_edges.h): the traced and simplified chains, library-owned host arrays."""
    _fields_ = [("n_chains", C.c_uint64), ("n_vertices", C.c_uint64), ("n_kept", C.c_uint64), ("chain_off", u64p),
                ("chain_node", u32p), ("chain_flags", u32p), ("s_off", u64p), ("s_node", u32p), ("length", f32p)]


class DeviceEdgeChains(C.Structure):
    """eg3d_device_edge_chains (include/eg3d/edges.h): the same, the pointers into HBM."""
    _fields_ = [("n_chains", C.c_uint64), ("n_vertices", C.c_uint64), ("n_kept", C.c_uint64), ("chain_off", C.c_void_p),
                ("chain_node", C.c_void_p), ("chain_flags", C.c_void_p), ("s_off", C.c_void_p), ("s_node", C.c_void_p),
                ("length", C.c_void_p)]


class EdgesStats(C.Structure):
    """eg3d_edges_stats (include/eg3d/host_edges.h): struct_size is set to the size of this mirror by its user before the call."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_chains", C.c_uint64), ("n_rings", C.c_uint64),
                ("n_loops_dropped", C.c_uint64), ("n_vertices_in", C.c_uint64), ("n_vertices_kept", C.c_uint64),
                ("longest_chain", C.c_uint64), ("ms_trace", C.c_float), ("ms_simplify", C.c_float), ("ms_copy", C.c_float),
                ("reserved2", C.c_float)]


class CloudIndexStats(C.Structure):
    """eg3d_cloud_index_stats (include/eg3d/host_nearest.hpp): struct_size is set to the size of this mirror by its user."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_points", C.c_uint64), ("n_dropped", C.c_uint64),
                ("n_nonfinite", C.c_uint64), ("n_indexed", C.c_uint64), ("n_cells", C.c_uint64), ("max_cell_points", C.c_uint64),
                ("origin", C.c_float * 3), ("cell", C.c_float), ("dims", C.c_uint32 * 3), ("reserved2", C.c_uint32),
                ("ms_build", C.c_float), ("ms_copy", C.c_float)]


class NearestStats(C.Structure):
    """eg3d_nearest_stats (include/eg3d/host_nearest.hpp): the thresholds in, the figures out."""
    _fields_ = [("struct_size", C.c_uint32), ("n_thresholds", C.c_uint32), ("thresholds", C.c_float * 8), ("n_queries", C.c_uint64),
                ("n_dropped", C.c_uint64), ("n_nonfinite", C.c_uint64), ("n_within", C.c_uint64), ("n_below", C.c_uint64 * 8),
                ("sum_q32", C.c_uint64), ("min_d2", C.c_float), ("max_d2", C.c_float), ("median_d2", C.c_float),
                ("ms_kernel", C.c_float), ("ms_copy", C.c_float), ("reserved", C.c_float)]


class EdgemapParams(C.Structure):
    """eg3d_edgemap_params (include/eg3d/host_edgemap.hh): struct_size is set to the size of this mirror by its user."""
    _fields_ = [("struct_size", C.c_uint32), ("low", C.c_int32), ("high", C.c_int32), ("smooth_passes", C.c_int32), ("l2", C.c_int32),
                ("reserved", C.c_uint32)]


class EdgemapStats(C.Structure):
    """eg3d_edgemap_stats (include/eg3d/host_edgemap.hh): the counts and the times of a call."""
    _fields_ = [("struct_size", C.c_uint32), ("n_views", C.c_uint32), ("n_pixels", C.c_uint64), ("n_candidates", C.c_uint64),
                ("n_strong", C.c_uint64), ("n_edges", C.c_uint64), ("hysteresis_rounds", C.c_uint32), ("reserved", C.c_uint32),
                ("ms_upload", C.c_float), ("ms_kernel", C.c_float), ("ms_hysteresis", C.c_float), ("ms_copy", C.c_float)]


def edgemap_call(fn, images, low, high, smooth_passes, l2):
    """What api.edge_maps and host.edge_maps share: `fn(n_views, width*, height*, rgb**, params*, masks**, stats*)` is the
    native call (the device index already bound). `images`: a sequence of uint8 [H, W, 3] arrays, which may differ in size.
    Returns rc, (masks: a list of uint8 [H, W] arrays, stats dict). The shapes are checked here, because the C side cannot
    know an array's length; the values are the library's to refuse."""
    imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
    for im in imgs:
        if im.ndim != 3 or im.shape[2] != 3:
            raise ValueError("an image must be [H, W, 3] uint8, not %r" % (im.shape,))
    n = len(imgs)
    w = np.array([im.shape[1] for im in imgs], np.int32)
    h = np.array([im.shape[0] for im in imgs], np.int32)
    masks = [np.zeros(im.shape[:2], np.uint8) for im in imgs]
    in_p = (u8p * max(n, 1))(*[np_ptr(im, C.c_uint8) for im in imgs])
    out_p = (u8p * max(n, 1))(*[np_ptr(m, C.c_uint8) for m in masks])
    params = EdgemapParams(struct_size=C.sizeof(EdgemapParams), low=int(low), high=int(high), smooth_passes=int(smooth_passes),
                           l2=1 if l2 else 0)
    st = EdgemapStats(struct_size=C.sizeof(EdgemapStats))
    rc = fn(n, np_ptr(w, C.c_int32), np_ptr(h, C.c_int32), in_p, C.byref(params), out_p, C.byref(st))
    stats = {f: int(getattr(st, f)) for f in ("n_views", "n_pixels", "n_candidates", "n_strong", "n_edges", "hysteresis_rounds")}
    stats.update({f: float(getattr(st, f)) for f in ("ms_upload", "ms_kernel", "ms_hysteresis", "ms_copy")})
    return rc, (masks, stats)


def cloud_index_stats_to_dict(st):
    """The figures of a CloudIndexStats: counts as ints, origin float32 [3], dims [3] ints, cell, the times."""
    d = {f: int(getattr(st, f)) for f in ("n_points", "n_dropped", "n_nonfinite", "n_indexed", "n_cells", "max_cell_points")}
    d.update(origin=np.array(st.origin[:], np.float32), dims=[int(v) for v in st.dims[:]], cell=np.float32(st.cell),
             ms_build=st.ms_build, ms_copy=st.ms_copy)
    return d


def nearest_stats_new(thresholds=()):
    """A NearestStats that carries `thresholds` in (as float32). Of more than 8 only the count travels, which the library
    refuses."""
    t = np.asarray(thresholds, np.float32).reshape(-1)
    st = NearestStats(struct_size=C.sizeof(NearestStats), n_thresholds=len(t))
    for k in range(min(len(t), 8)):
        st.thresholds[k] = float(t[k])
    return st


def nearest_stats_to_dict(st, max_dist):
    """The figures of a NearestStats: the counts and sum_q32 as ints, n_below for the thresholds given, min_d2 / max_d2 /
    median_d2 as float32, and — distances — mean (FP64, sum_q32 * max_dist / 2^32 / n_within) and median (sqrt of
    median_d2 in FP64); both nan for an empty within set."""
    nt = min(int(st.n_thresholds), 8)
    d = {f: int(getattr(st, f)) for f in ("n_queries", "n_dropped", "n_nonfinite", "n_within", "sum_q32")}
    d["n_below"] = [int(v) for v in st.n_below[:nt]]
    d["thresholds"] = np.array(st.thresholds[:nt], np.float32)
    for f in ("min_d2", "max_d2", "median_d2"):
        d[f] = np.float32(getattr(st, f))
    w = d["n_within"]
    d["mean"] = d["sum_q32"] * float(np.float32(max_dist)) / 4294967296.0 / w if w else float("nan")
    d["median"] = float(np.sqrt(np.float64(d["median_d2"]))) if w else float("nan")
    d["ms_kernel"], d["ms_copy"] = st.ms_kernel, st.ms_copy
    return d


def edge_chains_to_dict(c, stats=None):
    """The arrays of an EdgeChains as numpy copies: chain_off, chain_node, flags, s_off, s_node, length (+ stats)."""
    n = int(c.n_chains)
    d = {"chain_off": as_np(c.chain_off, n + 1, np.uint64), "chain_node": as_np(c.chain_node, int(c.n_vertices), np.uint32),
         "flags": as_np(c.chain_flags, n, np.uint32), "s_off": as_np(c.s_off, n + 1, np.uint64),
         "s_node": as_np(c.s_node, int(c.n_kept), np.uint32), "length": as_np(c.length, n, np.float32)}
    if stats is not None:
        d["stats"] = {f[0]: getattr(stats, f[0]) for f in EdgesStats._fields_ if not f[0].startswith("reserved")}
    return d


class EdgeChainsArrays:
    """Owns numpy copies of a chains dict (as edge_chains_to_dict gives it) and exposes an EdgeChains struct over them."""

    def __init__(self, d):
        self.a = {"chain_off": np.ascontiguousarray(d["chain_off"], np.uint64), "chain_node": np.ascontiguousarray(d["chain_node"], np.uint32),
                  "flags": np.ascontiguousarray(d["flags"], np.uint32), "s_off": np.ascontiguousarray(d["s_off"], np.uint64),
                  "s_node": np.ascontiguousarray(d["s_node"], np.uint32), "length": np.ascontiguousarray(d["length"], np.float32)}
        a = self.a
        n = len(a["flags"])
        if len(a["chain_off"]) != n + 1 or len(a["s_off"]) != n + 1 or len(a["length"]) != n:
            raise ValueError("chains: the arrays do not agree on the number of chains")
        if int(a["chain_off"][-1]) != len(a["chain_node"]) or int(a["s_off"][-1]) != len(a["s_node"]):
            raise ValueError("chains: the offsets do not end at the length of their array")
        if np.any(np.diff(a["s_off"].astype(np.int64)) < 0):
            raise ValueError("chains: s_off does not ascend")
        self.c = EdgeChains(n, len(a["chain_node"]), len(a["s_node"]), np_ptr(a["chain_off"], C.c_uint64),
                            np_ptr(a["chain_node"], C.c_uint32), np_ptr(a["flags"], C.c_uint32), np_ptr(a["s_off"], C.c_uint64),
                            np_ptr(a["s_node"], C.c_uint32), np_ptr(a["length"], C.c_float))


class EdgesGraphArrays:
    """Owns numpy copies of the geometric half of a graph dict (n_nodes, n_polylines, node_X, pl_start, pl_end, conn_off,
    conn_pl) and exposes a Graph3D struct over them for the edge-chain entry points. The C struct carries no array lengths:
    node_X, pl_start, pl_end and conn_off are held to the counts here (ValueError); conn_pl is padded with the invalid id
    0xFFFFFFFF up to 2 * n_polylines entries, so that whatever offsets the C side accepts, it reads inside the array."""

    def __init__(self, g):
        nn, npl = int(g["n_nodes"]), int(g["n_polylines"])
        X = np.ascontiguousarray(g["node_X"], np.float32).reshape(-1)
        ps, pe = np.ascontiguousarray(g["pl_start"], np.uint32).reshape(-1), np.ascontiguousarray(g["pl_end"], np.uint32).reshape(-1)
        off = np.ascontiguousarray(g["conn_off"], np.uint64).reshape(-1)
        cpl = np.ascontiguousarray(g["conn_pl"], np.uint32).reshape(-1)
        for name, a, n in (("node_X", X, 3 * nn), ("pl_start", ps, npl), ("pl_end", pe, npl), ("conn_off", off, nn + 1)):
            if a.size != n:
                raise ValueError("graph: %s holds %d values where its counts say %d" % (name, a.size, n))
        if cpl.size < 2 * npl:
            cpl = np.concatenate([cpl, np.full(2 * npl - cpl.size, 0xFFFFFFFF, np.uint32)])
        self.a = (X, ps, pe, off, cpl)
        self.c = Graph3D()
        self.c.n_nodes = self.c.n_real_nodes = nn
        self.c.n_polylines = npl
        self.c.node_X = np_ptr(X, C.c_float) if X.size else None
        self.c.pl_start = np_ptr(ps, C.c_uint32) if npl else None
        self.c.pl_end = np_ptr(pe, C.c_uint32) if npl else None
        self.c.conn_off = np_ptr(off, C.c_uint64)
        self.c.conn_pl = np_ptr(cpl, C.c_uint32) if cpl.size else None


class ImageArgs:
    """Owns what eg3d_upload_images / eg3d_host_colour_points take for `images`: a sequence with one entry per view, an
    [H, W, 3] uint8 array (RGB) or None for a view without an image."""

    def __init__(self, images):
        self.arrays = []
        for im in images:
            if im is not None:
                im = np.ascontiguousarray(im, np.uint8)
                if im.ndim != 3 or im.shape[2] != 3:
                    raise ValueError("an image is an [H, W, 3] uint8 array")
            self.arrays.append(im)
        self.n = len(self.arrays)
        self.width = np.array([0 if a is None else a.shape[1] for a in self.arrays] or [0], np.int32)
        self.height = np.array([0 if a is None else a.shape[0] for a in self.arrays] or [0], np.int32)
        self.rgb = (u8p * max(self.n, 1))()
        for v, a in enumerate(self.arrays):
            if a is not None:
                self.rgb[v] = a.ctypes.data_as(u8p)

    def args(self):
        return self.n, np_ptr(self.width, C.c_int32), np_ptr(self.height, C.c_int32), self.rgb


class EdgePoints(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("n_obs", C.c_uint64), ("X", f32p), ("obs_off", u64p),
                ("obs_view", i32p), ("obs_pl", u32p), ("obs_seg", u32p), ("obs_xy", f32p), ("key", u32p),
                ("n_tasks", C.c_uint64), ("n_hypotheses", C.c_uint64), ("n_chains", C.c_uint64),
                ("flags", C.c_uint32), ("_owner", C.c_void_p)]


class Candidates(C.Structure):
    _fields_ = [("n_sv", C.c_uint32), ("cand_off", u32p), ("cand_pl", u32p), ("start_off", u32p),
                ("start_pl", u32p), ("start_seg", u32p), ("start_xy", f32p), ("n_tasks", C.c_uint32),
                ("task_sv", u32p), ("task_hit", u32p), ("task_list_off", u32p), ("list_off", u32p),
                ("hit_pl", u32p), ("hit_seg", u32p), ("hit_xy", f32p), ("_owner", C.c_void_p)]


class MatchedIntervals(C.Structure):
    """eg3d_matched_intervals: the matched_polyline_intervals CSR of a graph (host or device pointers)."""
    _fields_ = [("struct_size", C.c_uint32), ("on_device", C.c_int32), ("n_scene_polylines", C.c_uint64),
                ("iv_off", C.c_void_p), ("iv_start_seg", C.c_void_p), ("iv_start_xy", C.c_void_p),
                ("iv_end_seg", C.c_void_p), ("iv_end_xy", C.c_void_p)]


class MatchedIntervalsArrays:
    """Owns what an eg3d_matched_intervals points at. `g` is the dict of a host graph (host.replay_matches,
    Context.replay_device) — numpy copies are kept here — or a DeviceGraph3D (Context.replay_device(to_host=False)),
    whose arrays stay where they are: the context that built them must not have replaced them since."""

    def __init__(self, g):
        if isinstance(g, DeviceGraph3D):
            self.a = None
            self.c = MatchedIntervals(C.sizeof(MatchedIntervals), 1, int(g.n_scene_polylines), g.iv_off, g.iv_start_seg,
                                      g.iv_start_xy, g.iv_end_seg, g.iv_end_xy)
            return
        pad = lambda k, t, w: np.ascontiguousarray(g[k], t).reshape(-1) if len(g[k]) else np.zeros(w, t)
        self.a = {"iv_off": np.ascontiguousarray(g["iv_off"], np.uint64),
                  "iv_start_seg": pad("iv_start_seg", np.uint32, 1), "iv_start_xy": pad("iv_start_xy", np.float32, 2),
                  "iv_end_seg": pad("iv_end_seg", np.uint32, 1), "iv_end_xy": pad("iv_end_xy", np.float32, 2)}
        a = self.a
        self.c = MatchedIntervals(C.sizeof(MatchedIntervals), 0, int(g.get("n_scene_polylines", len(a["iv_off"]) - 1)),
                                  a["iv_off"].ctypes.data, a["iv_start_seg"].ctypes.data, a["iv_start_xy"].ctypes.data,
                                  a["iv_end_seg"].ctypes.data, a["iv_end_xy"].ctypes.data)


class SetCandidates(C.Structure):
    """eg3d_set_candidates (library-owned; eg3d_free_set_candidates)."""
    _fields_ = [("n_tasks", C.c_uint32), ("task_view", i32p), ("task_pl", u32p), ("task_seg", u32p), ("task_xy", f32p),
                ("list_off", u64p), ("hit_pl", u32p), ("hit_seg", u32p), ("hit_xy", f32p),
                ("n_samples_skipped", C.c_uint64), ("n_hits_filtered", C.c_uint64), ("_owner", C.c_void_p)]


def set_candidates_to_dict(c, n_views):
    nt = int(c.n_tasks)
    list_off = as_np(c.list_off, nt * n_views + 1, np.uint64)
    nh = int(list_off[-1])
    return {"n_tasks": nt, "task_view": as_np(c.task_view, nt, np.int32), "task_pl": as_np(c.task_pl, nt, np.uint32),
            "task_seg": as_np(c.task_seg, nt, np.uint32), "task_xy": as_np(c.task_xy, 2 * nt, np.float32).reshape(nt, 2),
            "list_off": list_off, "hit_pl": as_np(c.hit_pl, nh, np.uint32), "hit_seg": as_np(c.hit_seg, nh, np.uint32),
            "hit_xy": as_np(c.hit_xy, 2 * nh, np.float32).reshape(nh, 2),
            "n_samples_skipped": int(c.n_samples_skipped), "n_hits_filtered": int(c.n_hits_filtered)}


class StageTimes(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_candidates", C.c_float), ("ms_epipolar", C.c_float),
                ("ms_hypotheses", C.c_float), ("ms_select", C.c_float), ("ms_expand", C.c_float),
                ("ms_emit", C.c_float), ("bytes_algorithmic", C.c_uint64), ("ms_slowest_chain", C.c_float)]


class DeviceEdgePoints(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("n_obs", C.c_uint64), ("X", C.c_void_p), ("obs_off", C.c_void_p),
                ("obs_view", C.c_void_p), ("obs_pl", C.c_void_p), ("obs_seg", C.c_void_p), ("obs_xy", C.c_void_p),
                ("key", C.c_void_p), ("complete", C.c_int32)]


class FilterStats(C.Structure):
    """eg3d_filter_stats: struct_size is set to the size of this mirror by its user before the call."""
    _fields_ = [("struct_size", C.c_uint32), ("threshold", C.c_int32), ("n_points_in", C.c_uint64),
                ("n_masked_in", C.c_uint64), ("n_gn_inliers", C.c_uint64), ("n_kept", C.c_uint64),
                ("n_obs_kept", C.c_uint64), ("ms_filter", C.c_float), ("ms_compact", C.c_float), ("ms_copy", C.c_float)]


class DedupStats(C.Structure):
    """eg3d_dedup_stats: struct_size is set to the size of this mirror by its user before the call."""
    _fields_ = [("struct_size", C.c_uint32), ("threshold", C.c_int32), ("n_points_in", C.c_uint64),
                ("n_dedup_kept", C.c_uint64), ("n_gn_inliers", C.c_uint64), ("n_kept", C.c_uint64),
                ("n_obs_kept", C.c_uint64), ("ms_dedup", C.c_float), ("ms_filter", C.c_float), ("ms_compact", C.c_float),
                ("ms_copy", C.c_float)]


class DeviceGraph3D(C.Structure):
    """eg3d_device_graph3d: the members of eg3d_graph3d, the pointers into HBM."""
    _fields_ = [("n_nodes", C.c_uint64), ("n_real_nodes", C.c_uint64), ("node_X", C.c_void_p), ("node_point", C.c_void_p),
                ("n_polylines", C.c_uint64), ("pl_start", C.c_void_p), ("pl_end", C.c_void_p), ("conn_off", C.c_void_p),
                ("conn_pl", C.c_void_p), ("n_scene_polylines", C.c_uint64), ("iv_off", C.c_void_p),
                ("iv_start_seg", C.c_void_p), ("iv_start_xy", C.c_void_p), ("iv_end_seg", C.c_void_p),
                ("iv_end_xy", C.c_void_p)]


class ReplayStats(C.Structure):
    """eg3d_replay_stats: struct_size is set to the size of this mirror by its user before the call."""
    _fields_ = [("struct_size", C.c_uint32), ("n_pairs", C.c_uint64), ("n_nodes", C.c_uint64), ("n_polylines", C.c_uint64),
                ("n_intervals", C.c_uint64), ("table_slots", C.c_uint64), ("ms_graph", C.c_float),
                ("ms_intervals", C.c_float), ("ms_copy", C.c_float)]


class PolylineMatches(C.Structure):
    """eg3d_polyline_matches (library-owned; eg3d_free_polyline_matches)."""
    _fields_ = [("n_refpoints", C.c_uint32), ("refpoints", u32p), ("n_sets", C.c_uint32), ("row_off", u32p), ("pl_ids", u32p)]


class PolymatchStats(C.Structure):
    """eg3d_polymatch_stats: struct_size is set to the size of this mirror by its user before the call."""
    _fields_ = [("struct_size", C.c_uint32), ("n_entries", C.c_uint64), ("n_accepted", C.c_uint64), ("n_nodes", C.c_uint64),
                ("n_sets", C.c_uint64), ("ms_grid", C.c_float), ("ms_search", C.c_float), ("ms_components", C.c_float),
                ("ms_copy", C.c_float)]


class Simgraph(C.Structure):
    """eg3d_simgraph (library-owned; eg3d_free_simgraph)."""
    _fields_ = [("n_nodes", C.c_uint32), ("node_view", u32p), ("node_pl", u32p), ("adj_off", u32p), ("adj_node", u32p),
                ("adj_w", f32p), ("seed_begin", C.c_uint32), ("n_points", C.c_uint32), ("point_weight", f32p),
                ("cp_off", u32p), ("cp_view", u32p), ("cp_pl", u32p), ("n_polylines", C.c_uint32), ("cr_off", u32p),
                ("cr_point", u32p)]


class SimgraphStats(C.Structure):
    """eg3d_simgraph_stats: struct_size is set to the size of this mirror by its user before the call."""
    _fields_ = [("struct_size", C.c_uint32), ("n_entries", C.c_uint64), ("n_nodes", C.c_uint64), ("n_edges", C.c_uint64),
                ("n_pair_instances", C.c_uint64), ("n_chunks", C.c_uint64), ("ms_grid", C.c_float), ("ms_search", C.c_float),
                ("ms_graph", C.c_float), ("ms_weights", C.c_float), ("ms_copy", C.c_float)]


class LouvainParams(C.Structure):
    """eg3d_louvain_params: a field of 0 is its default."""
    _fields_ = [("struct_size", C.c_uint32), ("max_phases", C.c_uint32), ("max_sweeps", C.c_uint32),
                ("sweep_threshold", C.c_double), ("phase_threshold", C.c_double)]


class Communities(C.Structure):
    """eg3d_communities (library-owned; eg3d_free_communities)."""
    _fields_ = [("n_nodes", C.c_uint32), ("ids", C.POINTER(C.c_int64)), ("n_communities", C.c_uint32)]


class LouvainStats(C.Structure):
    """eg3d_louvain_stats: struct_size is set to the size of this mirror by its user before the call."""
    _fields_ = [("struct_size", C.c_uint32), ("n_phases", C.c_uint32), ("n_sweeps", C.c_uint32), ("n_communities", C.c_uint32),
                ("n_isolated", C.c_uint32), ("n_overflow_rows", C.c_uint64), ("total_q", C.c_uint64), ("numer_hi", C.c_uint64),
                ("numer_lo", C.c_uint64), ("modularity", C.c_double), ("ms_upload", C.c_float), ("ms_sweeps", C.c_float),
                ("ms_coarsen", C.c_float), ("ms_copy", C.c_float)]


class FundParams(C.Structure):
    """eg3d_fund_params: a field of 0 is its default."""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("rng_seed", C.c_uint64), ("fit_budget", C.c_uint32),
                ("stage_points", C.c_uint32)]


class FundStats(C.Structure):
    """eg3d_fund_stats: struct_size is set to the size of this mirror by its user before the call."""
    _fields_ = [("struct_size", C.c_uint32), ("n_pairs_valid", C.c_uint32), ("n_pairs_failed", C.c_uint32), ("n_chunks", C.c_uint32),
                ("n_common_total", C.c_uint64), ("n_fits", C.c_uint64), ("n_fits_degenerate", C.c_uint64),
                ("n_exact_medians", C.c_uint64), ("ms_upload", C.c_float), ("ms_lists", C.c_float), ("ms_samples", C.c_float),
                ("ms_fits", C.c_float), ("ms_select", C.c_float), ("ms_refit", C.c_float), ("ms_copy", C.c_float)]


def fund_call(fn, n_views, seeds, iterations, rng_seed, fit_budget, stage_points):
    """What api.estimate_fundamental and host.estimate_fundamental share: `fn(n_views, seeds*, params*, F, valid, n_common,
    stats*)` is the native call (the device index already bound). `seeds` is a POINTER(Seeds) / Seeds, or (trk_off, trk_view,
    trk_xy). Returns rc, (F [V,V,9] f64, valid [V,V] u8, n_common [V,V] u32, stats dict)."""
    keep = None
    if isinstance(seeds, (tuple, list)):
        off = np.ascontiguousarray(seeds[0], np.uint32)
        view = np.ascontiguousarray(seeds[1] if len(seeds[1]) else [0], np.int32)
        xy = np.ascontiguousarray(seeds[2] if len(seeds[2]) else [[0, 0]], np.float32)
        keep = (off, view, xy)
        seeds = C.pointer(Seeds(len(off) - 1, np_ptr(off, C.c_uint32), np_ptr(view, C.c_int32), np_ptr(xy, C.c_float)))
    elif isinstance(seeds, Seeds):
        seeds = C.pointer(seeds)
    V = max(int(n_views), 0)
    F = np.zeros((V, V, 9), np.float64)
    valid = np.zeros((V, V), np.uint8)
    ncom = np.zeros((V, V), np.uint32)
    pr = FundParams(C.sizeof(FundParams), int(iterations), int(rng_seed), int(fit_budget), int(stage_points))
    st = FundStats()
    st.struct_size = C.sizeof(FundStats)
    rc = fn(int(n_views), seeds, C.byref(pr), np_ptr(F, C.c_double), np_ptr(valid, C.c_uint8), np_ptr(ncom, C.c_uint32), C.byref(st))
    del keep
    return rc, (F, valid, ncom, {f[0]: getattr(st, f[0]) for f in FundStats._fields_})


def simgraph_to_dict(g):
    """Numpy copies of every array of an eg3d_simgraph."""
    nn, npt, npl = int(g.n_nodes), int(g.n_points), int(g.n_polylines)
    adj_off = as_np(g.adj_off, nn + 1, np.uint32)
    cp_off = as_np(g.cp_off, npt + 1, np.uint32)
    cr_off = as_np(g.cr_off, npl + 1, np.uint32)
    na, ncp, ncr = int(adj_off[-1]), int(cp_off[-1]), int(cr_off[-1])
    return {"n_nodes": nn, "node_view": as_np(g.node_view, nn, np.uint32), "node_pl": as_np(g.node_pl, nn, np.uint32),
            "adj_off": adj_off, "adj_node": as_np(g.adj_node, na, np.uint32), "adj_w": as_np(g.adj_w, na, np.float32),
            "seed_begin": int(g.seed_begin), "n_points": npt, "point_weight": as_np(g.point_weight, npt, np.float32),
            "cp_off": cp_off, "cp_view": as_np(g.cp_view, ncp, np.uint32), "cp_pl": as_np(g.cp_pl, ncp, np.uint32),
            "n_polylines": npl, "cr_off": cr_off, "cr_point": as_np(g.cr_point, ncr, np.uint32)}


class SimgraphArrays:
    """Owns numpy copies of a compatibility graph (a dict as returned by simgraph_to_dict / Context.similarity_graph) and
    exposes a Simgraph struct over them, for the host steps that consume one."""

    def __init__(self, d):
        u = lambda k: np.ascontiguousarray(d[k] if len(d[k]) else [0], np.uint32)
        f = lambda k: np.ascontiguousarray(d[k] if len(d[k]) else [0], np.float32)
        self.a = {k: u(k) for k in ("node_view", "node_pl", "adj_off", "adj_node", "cp_off", "cp_view", "cp_pl", "cr_off",
                                    "cr_point")}
        self.a.update({k: f(k) for k in ("adj_w", "point_weight")})
        a, p = self.a, np_ptr
        self.c = Simgraph(int(d["n_nodes"]), p(a["node_view"], C.c_uint32), p(a["node_pl"], C.c_uint32),
                          p(a["adj_off"], C.c_uint32), p(a["adj_node"], C.c_uint32), p(a["adj_w"], C.c_float),
                          int(d.get("seed_begin", 0)), int(d["n_points"]), p(a["point_weight"], C.c_float),
                          p(a["cp_off"], C.c_uint32), p(a["cp_view"], C.c_uint32), p(a["cp_pl"], C.c_uint32),
                          int(d["n_polylines"]), p(a["cr_off"], C.c_uint32), p(a["cr_point"], C.c_uint32))


class SynthConfig(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("n_seeds", C.c_uint32), ("n_curves", C.c_int32),
                ("rng_seed", C.c_uint64), ("max_track", C.c_int32), ("obs_noise_px", C.c_float),
                ("vtx_noise_px", C.c_float), ("invalid_frac", C.c_float), ("seed_offset_px", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32), ("focal", C.c_float), ("ppx", C.c_float),
                ("ppy", C.c_float)]


def as_np(ptr, n, dtype):
    """Copy n elements behind a ctypes pointer into a numpy array."""
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(int(n),)).astype(dtype, copy=True)


def np_ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


class PlgView(C.Structure):
    """eg3d_plg_view (include/eg3d_host.h): the polyline graph of one view."""
    _fields_ = [("n_polylines", C.c_uint32), ("pl_vtx_off", u32p), ("vtx_xy", f32p), ("pl_start", u32p),
                ("pl_end", u32p), ("pl_valid", u8p), ("n_nodes", C.c_uint32), ("node_xy", f32p)]


def plg_view_to_dict(v):
    n, nn = int(v.n_polylines), int(v.n_nodes)
    off = as_np(v.pl_vtx_off, n + 1, np.uint32)
    nv = int(off[-1]) if n else 0
    return {"n_polylines": n, "n_nodes": nn, "pl_vtx_off": off,
            "vtx_xy": as_np(v.vtx_xy, 2 * nv, np.float32).reshape(nv, 2),
            "pl_start": as_np(v.pl_start, n, np.uint32), "pl_end": as_np(v.pl_end, n, np.uint32),
            "pl_valid": as_np(v.pl_valid, n, np.uint8), "node_xy": as_np(v.node_xy, 2 * nn, np.float32).reshape(nn, 2)}


class Graph3D(C.Structure):
    """eg3d_graph3d (include/eg3d_host.h): the PLGMatchesManager replay (row a17)."""
    _fields_ = [("n_nodes", C.c_uint64), ("n_real_nodes", C.c_uint64), ("node_X", f32p),
                ("node_point", C.POINTER(C.c_uint64)), ("n_polylines", C.c_uint64), ("pl_start", u32p),
                ("pl_end", u32p), ("conn_off", C.POINTER(C.c_uint64)), ("conn_pl", u32p),
                ("n_scene_polylines", C.c_uint64), ("iv_off", C.POINTER(C.c_uint64)), ("iv_start_seg", u32p),
                ("iv_start_xy", f32p), ("iv_end_seg", u32p), ("iv_end_xy", f32p)]


def graph3d_to_dict(g):
    nn, npl, nsp = int(g.n_nodes), int(g.n_polylines), int(g.n_scene_polylines)
    conn_off = as_np(g.conn_off, nn + 1, np.uint64)
    iv_off = as_np(g.iv_off, nsp + 1, np.uint64)
    ni = int(iv_off[-1]) if nsp else 0
    nc = int(conn_off[-1]) if nn else 0
    return {
        "n_nodes": nn, "n_real_nodes": int(g.n_real_nodes), "n_polylines": npl,
        "node_X": as_np(g.node_X, 3 * nn, np.float32).reshape(nn, 3),
        "node_point": as_np(g.node_point, nn, np.uint64),
        "pl_start": as_np(g.pl_start, npl, np.uint32), "pl_end": as_np(g.pl_end, npl, np.uint32),
        "conn_off": conn_off, "conn_pl": as_np(g.conn_pl, nc, np.uint32),
        "iv_off": iv_off, "iv_start_seg": as_np(g.iv_start_seg, ni, np.uint32),
        "iv_start_xy": as_np(g.iv_start_xy, 2 * ni, np.float32).reshape(ni, 2),
        "iv_end_seg": as_np(g.iv_end_seg, ni, np.uint32),
        "iv_end_xy": as_np(g.iv_end_xy, 2 * ni, np.float32).reshape(ni, 2),
    }


GRAPH3D_ARRAYS = (("node_X", np.float32), ("node_point", np.uint64), ("pl_start", np.uint32), ("pl_end", np.uint32),
                  ("conn_off", np.uint64), ("conn_pl", np.uint32), ("iv_off", np.uint64), ("iv_start_seg", np.uint32),
                  ("iv_start_xy", np.float32), ("iv_end_seg", np.uint32), ("iv_end_xy", np.float32))


def graph3d_lengths_check(g, a):
    """The C struct carries no array lengths: a graph dict whose arrays (`a`: flattened) are shorter or longer than its
    counts and its interval offsets say is refused here, with ValueError, before a pointer to them is handed on. conn_* are
    not held to it (the merge does not read them)."""
    nn, npl = int(g["n_nodes"]), int(g["n_polylines"])
    ni = int(a["iv_off"][-1]) if a["iv_off"].size else -1
    want = {"node_X": 3 * nn, "node_point": nn, "pl_start": npl, "pl_end": npl, "iv_start_seg": ni, "iv_end_seg": ni,
            "iv_start_xy": 2 * ni, "iv_end_xy": 2 * ni}
    for k, n in want.items():
        if a[k].size != n:
            raise ValueError("graph: %s holds %d values where its counts say %d" % (k, a[k].size, n))


class Graph3DArrays:
    """Owns numpy copies of a graph (a dict as returned by graph3d_to_dict) and exposes a Graph3D struct over them, for
    the steps that consume a graph (host.ReplayState.merge). n_scene_polylines is what iv_off says."""

    def __init__(self, g):
        self.a = {k: np.ascontiguousarray(g[k], t).reshape(-1) for k, t in GRAPH3D_ARRAYS}
        a = self.a
        graph3d_lengths_check(g, a)
        self.c = Graph3D()
        self.c.n_nodes, self.c.n_real_nodes, self.c.n_polylines = int(g["n_nodes"]), int(g["n_real_nodes"]), int(g["n_polylines"])
        self.c.n_scene_polylines = int(g.get("n_scene_polylines", len(a["iv_off"]) - 1))
        for k, t in GRAPH3D_ARRAYS:
            setattr(self.c, k, np_ptr(a[k], np.ctypeslib.as_ctypes_type(t)) if a[k].size else None)


class EdgePointsArrays:
    """Owns numpy copies of an edge-point cloud (a dict as returned by edgepoints_to_dict) and
    exposes an EdgePoints struct over them, for the host steps that consume a cloud."""

    def __init__(self, d):
        self.a = {"X": np.ascontiguousarray(d["X"], np.float32), "obs_off": np.ascontiguousarray(d["obs_off"], np.uint64),
                  "obs_view": np.ascontiguousarray(d["obs_view"], np.int32),
                  "obs_pl": np.ascontiguousarray(d["obs_pl"], np.uint32),
                  "obs_seg": np.ascontiguousarray(d["obs_seg"], np.uint32),
                  "obs_xy": np.ascontiguousarray(d["obs_xy"], np.float32),
                  "key": np.ascontiguousarray(d["key"], np.uint32)}
        a = self.a
        n = len(a["obs_off"]) - 1
        self.c = EdgePoints(n, int(a["obs_off"][-1]) if n >= 0 else 0, np_ptr(a["X"], C.c_float),
                            np_ptr(a["obs_off"], C.c_uint64), np_ptr(a["obs_view"], C.c_int32),
                            np_ptr(a["obs_pl"], C.c_uint32), np_ptr(a["obs_seg"], C.c_uint32),
                            np_ptr(a["obs_xy"], C.c_float), np_ptr(a["key"], C.c_uint32), 0, 0, 0, 0, None)


def edgepoints_to_dict(e):
    n, m = int(e.n_points), int(e.n_obs)
    return {
        "n_points": n, "n_obs": m,
        "X": as_np(e.X, 3 * n, np.float32).reshape(n, 3),
        "obs_off": as_np(e.obs_off, n + 1, np.uint64),
        "obs_view": as_np(e.obs_view, m, np.int32),
        "obs_pl": as_np(e.obs_pl, m, np.uint32),
        "obs_seg": as_np(e.obs_seg, m, np.uint32),
        "obs_xy": as_np(e.obs_xy, 2 * m, np.float32).reshape(m, 2),
        "key": as_np(e.key, 4 * n, np.uint32).reshape(n, 4),
        "n_tasks": int(e.n_tasks), "n_hypotheses": int(e.n_hypotheses), "n_chains": int(e.n_chains),
        "flags": int(e.flags),
    }


def candidates_to_dict(c):
    nsv, nt = int(c.n_sv), int(c.n_tasks)
    cand_off = as_np(c.cand_off, nsv + 1, np.uint32)
    start_off = as_np(c.start_off, nsv + 1, np.uint32)
    task_list_off = as_np(c.task_list_off, nt + 1, np.uint32)
    nl = int(task_list_off[-1]) if nt else 0
    list_off = as_np(c.list_off, nl + 1, np.uint32)
    nh = int(list_off[-1]) if nl else 0
    ns = int(start_off[-1]) if nsv else 0
    return {
        "n_sv": nsv, "n_tasks": nt, "cand_off": cand_off,
        "cand_pl": as_np(c.cand_pl, int(cand_off[-1]) if nsv else 0, np.uint32),
        "start_off": start_off, "start_pl": as_np(c.start_pl, ns, np.uint32),
        "start_seg": as_np(c.start_seg, ns, np.uint32),
        "start_xy": as_np(c.start_xy, 2 * ns, np.float32).reshape(ns, 2),
        "task_sv": as_np(c.task_sv, nt, np.uint32), "task_hit": as_np(c.task_hit, nt, np.uint32),
        "task_list_off": task_list_off, "list_off": list_off,
        "hit_pl": as_np(c.hit_pl, nh, np.uint32), "hit_seg": as_np(c.hit_seg, nh, np.uint32),
        "hit_xy": as_np(c.hit_xy, 2 * nh, np.float32).reshape(nh, 2),
    }


# header of include/ -> {C struct: its mirror above}; tests/test_abi.py holds each to gcc's layout of the struct
MIRRORS = {
    "eg3d.h": {
        "eg3d_scene": Scene, "eg3d_seeds": Seeds, "eg3d_edgepoints": EdgePoints, "eg3d_candidates": Candidates,
        "eg3d_stage_times": StageTimes, "eg3d_polyline_sets": PolylineSets, "eg3d_matched_intervals": MatchedIntervals,
        "eg3d_set_candidates": SetCandidates, "eg3d_device_edgepoints": DeviceEdgePoints, "eg3d_filter_stats": FilterStats,
        "eg3d_dedup_stats": DedupStats, "eg3d_device_graph3d": DeviceGraph3D, "eg3d_replay_stats": ReplayStats,
        "eg3d_polyline_matches": PolylineMatches, "eg3d_polymatch_stats": PolymatchStats, "eg3d_simgraph": Simgraph,
        "eg3d_simgraph_stats": SimgraphStats, "eg3d_louvain_params": LouvainParams, "eg3d_communities": Communities,
        "eg3d_louvain_stats": LouvainStats, "eg3d_fund_params": FundParams, "eg3d_fund_stats": FundStats,
    },
    "eg3d_host.h": {"eg3d_synth_config": SynthConfig, "eg3d_plg_view": PlgView, "eg3d_graph3d": Graph3D},
    "eg3d_sets_device.h": {"eg3d_device_polyline_sets": DevicePolylineSets, "eg3d_items_call": ItemsCall,
                           "eg3d_sets_device_stats": SetsDeviceStats},
    "eg3d_triangulate.h": {"eg3d_tri_stats": TriStats},
    "eg3d_colour.h": {"eg3d_colour_stats": ColourStats},
    "eg3d_transform.h": {"eg3d_transform_stats": TransformStats},
    "eg3d_host_transform.h": {"eg3d_similarity_stats": SimilarityStats},
}
# the same for the headers in subdirectories of include/ (_cabi.EXT_HEADERS); tests/test_abi_edges.py holds these
MIRRORS_EXT = {
    "eg3d/edges.h": {"eg3d_device_edge_chains": DeviceEdgeChains},
    "eg3d/host_edges.h": {"eg3d_edge_chain_set": EdgeChains, "eg3d_edges_stats": EdgesStats},
}
# ... and for the .hpp ABI headers (_cabi.HPP_HEADERS); tests/test_abi_nearest.py holds these
MIRRORS_HPP = {
    "eg3d/host_nearest.hpp": {"eg3d_cloud_index_stats": CloudIndexStats, "eg3d_nearest_stats": NearestStats},
}
# ... and for the open registry (_cabi.OPEN_HEADERS: headers of any suffix the older tests do not pin); tests/test_abi_open.py
# holds these. The next header's structs are a row here.
MIRRORS_OPEN = {
    "eg3d/host_edgemap.hh": {"eg3d_edgemap_params": EdgemapParams, "eg3d_edgemap_stats": EdgemapStats},
}
