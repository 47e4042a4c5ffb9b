"""Python view of the C ABI (include/eg3d.h) in libeg3d.so — plumbing over ctypes.

There is no CPU fallback: constructing a Context without the built HIP library or without a
GPU raises. The class mirrors the reference call surface for the path:
  Context(scene)                     ~ PLGEdgeManager / PLGPCM3ViewsPLGFollowing construction
  Context.match_refpoints(seeds)     ~ plg_matching_from_refpoints_parallel(sfmd, em, cm, plgmm)
  Context.candidates(seeds)          ~ PLGEdgeManager::detect_nearby_intersections_and_correspondences_plgp
  Context.gn_filter(...)             ~ gaussNewtonFiltering(sfmd, inliers, gn_max_mse)
"""
import ctypes as C
import os

import numpy as np

from . import _cdefs as D
from ._cabi import EG3D, bind_library

_LIB = None


class Eg3dError(RuntimeError):
    pass


# include/eg3d_triangulate.h
TRI_FROM_SCRATCH, TRI_REFINE = 0, 1
TRI_FLAG_SHORT, TRI_FLAG_DEGENERATE = 1, 2
# include/eg3d_colour.h
COLOUR_FLAG_EMPTY = 1


def lib_path():
    # EG3D_LIB selects an alternative build of the same library (tuning experiments only)
    return os.environ.get("EG3D_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libeg3d.so")


def lib():
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise Eg3dError("libeg3d.so (HIP extension) is missing: run `python -m edgegraph3d_amd.build`. "
                            "There is no CPU fallback.")
        _LIB = bind_library(C.CDLL(path), "eg3d")
    return _LIB


# every symbol include/eg3d.h declares (the later headers' functions are in their tables in _cabi.py)
EXPORTED_SYMBOLS = list(EG3D)
ERR_TRANSFORM_NONFINITE, ERR_TRANSFORM_OVERLAP = -16, -17


def _check(rc, what):
    if rc != 0:
        err = Eg3dError("%s failed (rc=%d): %s" % (what, rc, lib().eg3d_last_error().decode()))
        err.code = rc   # (the C code: EG3D_ERR_*, and the codes of the later headers)
        raise err


def check_polyline_sets(n_sets, row_off, pl_ids, n_views):
    """eg3d_check_polyline_sets: the device-free checks of a polyline-sets CSR (row_off ascending, ids strictly ascending
    within every row). Raises Eg3dError if the sets are refused."""
    row_off = np.ascontiguousarray(row_off, np.uint32)
    pl_ids = np.ascontiguousarray(pl_ids if len(pl_ids) else [0], np.uint32)
    ps = D.PolylineSets(n_sets, D.np_ptr(row_off, C.c_uint32), D.np_ptr(pl_ids, C.c_uint32))
    _check(lib().eg3d_check_polyline_sets(C.byref(ps), n_views), "eg3d_check_polyline_sets")


def device_count():
    return int(lib().eg3d_device_count())


def estimate_fundamental(n_views, seeds, iterations=0, rng_seed=0, fit_budget=0, stage_points=0, device=0):
    """SURVEY N4 on the device (eg3d_estimate_fundamental, K12): the fundamental matrices of all ordered view pairs from
    the tracks, before any Context exists. `seeds` is a seeds pointer (Synth.seeds) or (trk_off, trk_view, trk_xy); 0 in a
    parameter is its default. Returns (F [V,V,9] f64, valid [V,V] u8, n_common [V,V] u32, stats dict) — bit for bit what
    host.estimate_fundamental returns."""
    L = lib()
    rc, out = D.fund_call(lambda *a: L.eg3d_estimate_fundamental(int(device), *a), n_views, seeds, iterations, rng_seed,
                          fit_budget, stage_points)
    _check(rc, "eg3d_estimate_fundamental")
    return out


def edge_maps(images, low, high, smooth_passes=1, l2=False, device=0):
    """The edge maps of the source images on the device (eg3d_edge_maps, K19), before any Context exists. `images`: a
    sequence of uint8 [H, W, 3] RGB arrays, which may differ in size; 0 <= low <= high <= 65535 bound the gradient
    magnitude (|gx| + |gy|, or with l2 its square against the squared bounds). Returns (masks, stats): one uint8 [H, W]
    mask per image, 1 = edge — what host.plg_from_mask takes — and the counts and times; bit for bit what host.edge_maps
    returns (include/eg3d/host_edgemap.hh states the rules)."""
    L = lib()
    rc, out = D.edgemap_call(lambda *a: L.eg3d_edge_maps(int(device), *a), images, low, high, smooth_passes, l2)
    _check(rc, "eg3d_edge_maps")
    return out


_HIP = None


def _hip():
    """The HIP runtime libeg3d.so itself is linked against (loaded once): the copy already in the process by its SONAME,
    the ROCm installation's otherwise."""
    global _HIP
    if _HIP is None:
        lib()   # (libeg3d.so first: its runtime is then the one the SONAME finds)
        try:
            hip = C.CDLL("libamdhip64.so.7")
        except OSError:
            hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipSetDevice.argtypes = [C.c_int]
        _HIP = hip
    return _HIP


class DeviceArray:
    """A block of HBM owned by Python (hipMalloc / hipFree): where callers place masks and receive the per-point results of
    the device-resident filter. `ptr` is the device address; numpy() copies it back. The memory is freed when the object
    is collected: keep the object, not just its `ptr`, for as long as a device view refers to it."""

    def __init__(self, nbytes, device=0):
        self.nbytes, self.device, self.ptr = int(nbytes), int(device), None
        p = C.c_void_p()
        if _hip().hipSetDevice(self.device) != 0 or _hip().hipMalloc(C.byref(p), max(self.nbytes, 256)) != 0:
            raise Eg3dError("hipMalloc(%d) failed" % self.nbytes)
        self.ptr = p.value

    def numpy(self, dtype, shape=None):
        a = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype)
        if a.nbytes and _hip().hipMemcpy(a.ctypes.data, C.c_void_p(self.ptr), a.nbytes, 2) != 0:
            raise Eg3dError("hipMemcpy from the device failed")
        return a.reshape(shape) if shape is not None else a

    def free(self):
        if self.ptr:
            _hip().hipFree(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_alloc(nbytes, device=0):
    return DeviceArray(nbytes, device)


def upload(array, device=0):
    """A numpy array copied into a fresh DeviceArray on `device`."""
    a = np.ascontiguousarray(array)
    d = DeviceArray(a.nbytes, device)
    if a.nbytes and _hip().hipMemcpy(C.c_void_p(d.ptr), a.ctypes.data, a.nbytes, 1) != 0:
        raise Eg3dError("hipMemcpy to the device failed")
    return d


def _dev_ptr(x):
    if x is None:
        return None
    return C.c_void_p(x.ptr if isinstance(x, DeviceArray) else int(x))


def points_cloud(X_dev, n_points):
    """A DeviceEdgePoints that views a bare [n_points, 3] float32 array on the device (a DeviceArray or a device address) as a
    whole cloud without observations: what the entry points of include/eg3d/nearest.hpp, which read only X, take
    (cloud_index, nearest_device). Keep the DeviceArray alive for as long as the view is used."""
    if isinstance(X_dev, DeviceArray) and X_dev.nbytes < 12 * int(n_points):
        raise ValueError("points_cloud: the array holds %d bytes, %d points need %d" % (X_dev.nbytes, n_points, 12 * int(n_points)))
    return D.DeviceEdgePoints(n_points=int(n_points), n_obs=0, X=_dev_ptr(X_dev), complete=1)


class CloudIndex:
    """A uniform-grid index over a reference point set on the device (include/eg3d/nearest.hpp), made by
    Context.cloud_index. `stats`: the figures of the build (n_indexed, n_cells, origin, dims, max_cell_points, ...). It
    holds device memory and works on its context's stream: close() it — or use it as a context manager — before the
    context is closed; it keeps the context alive until then."""

    def __init__(self, ctx, handle, stats):
        self._ctx, self._h, self.stats = ctx, handle, stats
        self.n_indexed, self.n_cells, self.cell = stats["n_indexed"], stats["n_cells"], stats["cell"]

    def close(self):
        if self._h:
            lib().eg3d_cloud_index_free(self._h)
            self._h, self._ctx = C.c_void_p(), None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# include/eg3d/host_nearest.hpp
NEAREST_NONE = 0xFFFFFFFF
ERR_NEAREST_CELL, ERR_NEAREST_MAXDIST, ERR_NEAREST_THRESHOLD, ERR_NEAREST_EXTENT, ERR_NEAREST_FOREIGN = -18, -19, -20, -21, -22


class Context:
    def __init__(self, scene_ptr, device=0, _handle=None):
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            _check(lib().eg3d_create(scene_ptr, device, C.byref(self._h)), "eg3d_create")
        nv, dv = C.c_int32(), C.c_int32()
        _check(lib().eg3d_context_info(self._h, C.byref(nv), C.byref(dv)), "eg3d_context_info")
        self.n_views, self.device = nv.value, dv.value

    def clone(self):
        """A context sharing this one's scene and resident seeds (own stream and work buffers)."""
        h = C.c_void_p()
        _check(lib().eg3d_clone(self._h, C.byref(h)), "eg3d_clone")
        return Context(None, _handle=h)

    def set_pipelining(self, lanes=0, units=0):
        """Sub-batches of one call kept in flight inside the library (eg3d_set_pipelining): lanes=1 switches it off."""
        _check(lib().eg3d_set_pipelining(self._h, lanes, units), "eg3d_set_pipelining")

    def probe_k3a_walks(self):
        """TEST-ONLY builds (variants/libeg3d_engine.so, timing builds): (walks the K3a walk service finished for a lane,
        64-segment passes they took) of this context's match calls since the last probe. The product library carries no
        probe: Eg3dError there."""
        L = lib()
        if not hasattr(L, "eg3d_probe_k3a_walks"):
            raise Eg3dError("eg3d_probe_k3a_walks: not in this library (test-only builds carry it)")
        L.eg3d_probe_k3a_walks.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
        out = (C.c_ulonglong * 2)()
        _check(L.eg3d_probe_k3a_walks(self._h, out), "eg3d_probe_k3a_walks")
        return int(out[0]), int(out[1])

    def close(self):
        if self._h:
            lib().eg3d_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def grid(self, view, which):
        ncols, nrows = C.c_uint32(), C.c_uint32()
        off, ids = D.u32p(), D.u32p()
        _check(lib().eg3d_get_grid(self._h, view, which, C.byref(ncols), C.byref(nrows), C.byref(off), C.byref(ids)),
               "eg3d_get_grid")
        n = ncols.value * nrows.value
        o = D.as_np(off, n + 1, np.uint32)
        return ncols.value, nrows.value, o, D.as_np(ids, int(o[-1]), np.uint32)

    def upload_seeds(self, seeds_ptr):
        _check(lib().eg3d_upload_seeds(self._h, seeds_ptr), "eg3d_upload_seeds")

    def match_resident(self, begin, end, device_only=False):
        e, tm = D.EdgePoints(), D.StageTimes()
        rc = lib().eg3d_match_resident(self._h, begin, end, 1 if device_only else 0, C.byref(e), C.byref(tm))
        _check(rc, "eg3d_match_resident")
        if device_only:
            d = {"n_points": int(e.n_points), "n_obs": int(e.n_obs), "n_tasks": int(e.n_tasks),
                 "n_hypotheses": int(e.n_hypotheses), "n_chains": int(e.n_chains), "flags": int(e.flags)}
        else:
            d = D.edgepoints_to_dict(e)
        lib().eg3d_free_edgepoints(C.byref(e))
        d["times"] = {f[0]: getattr(tm, f[0]) for f in D.StageTimes._fields_}
        return d

    def time_match_to_host(self, begin, end):
        """Wall seconds of ONE eg3d_match_resident(..., device_only=0) call at the C ABI (kernels + D2H of the
        cloud into caller-owned arrays), without this wrapper's conversion to numpy; returns (seconds, n_points)."""
        import time
        e, tm = D.EdgePoints(), D.StageTimes()
        t0 = time.perf_counter()
        rc = lib().eg3d_match_resident(self._h, begin, end, 0, C.byref(e), C.byref(tm))
        dt = time.perf_counter() - t0
        _check(rc, "eg3d_match_resident")
        n = int(e.n_points)
        lib().eg3d_free_edgepoints(C.byref(e))
        return dt, n

    def time_match_sets_to_host(self, n_sets, row_off, pl_ids):
        """The same for eg3d_match_polyline_sets: (seconds, n_points) of one call with device_only=0 at the C ABI."""
        import time
        row_off = np.ascontiguousarray(row_off, np.uint32)
        pl_ids = np.ascontiguousarray(pl_ids if len(pl_ids) else [0], np.uint32)
        ps = D.PolylineSets(n_sets, D.np_ptr(row_off, C.c_uint32), D.np_ptr(pl_ids, C.c_uint32))
        e, tm = D.EdgePoints(), D.StageTimes()
        t0 = time.perf_counter()
        rc = lib().eg3d_match_polyline_sets(self._h, C.byref(ps), 0, n_sets, 0, C.byref(e), C.byref(tm))
        dt = time.perf_counter() - t0
        _check(rc, "eg3d_match_polyline_sets")
        n = int(e.n_points)
        lib().eg3d_free_edgepoints(C.byref(e))
        return dt, n

    def match_refpoints(self, seeds_ptr, begin=0, end=None, device_only=False):
        if end is None:
            end = int(seeds_ptr.contents.n_seeds) if hasattr(seeds_ptr, "contents") else int(seeds_ptr.n_seeds)
        self.upload_seeds(seeds_ptr)
        return self.match_resident(begin, end, device_only)

    def match_polyline_sets(self, n_sets, row_off, pl_ids, begin=0, end=None, device_only=False, matched=None):
        """Pipelines 1-2 extractor: sets = CSR over rows (set * V + view) of polyline ids. `matched`: the
        graph whose matched intervals the extractor consults (eg3d_match_polyline_sets_matched) — the dict of a host graph
        (host.replay_matches, replay_device) or the DeviceGraph3D of replay_device(to_host=False) on this context; samples
        and epipolar hits inside a held interval are left out. None: no manager (eg3d_match_polyline_sets)."""
        if end is None:
            end = n_sets
        row_off = np.ascontiguousarray(row_off, np.uint32)
        pl_ids = np.ascontiguousarray(pl_ids if len(pl_ids) else [0], np.uint32)
        ps = D.PolylineSets(n_sets, D.np_ptr(row_off, C.c_uint32), D.np_ptr(pl_ids, C.c_uint32))
        e, tm = D.EdgePoints(), D.StageTimes()
        if matched is None:
            rc = lib().eg3d_match_polyline_sets(self._h, C.byref(ps), begin, end, 1 if device_only else 0, C.byref(e),
                                                C.byref(tm))
        else:
            m = matched if isinstance(matched, D.MatchedIntervalsArrays) else D.MatchedIntervalsArrays(matched)
            rc = lib().eg3d_match_polyline_sets_matched(self._h, C.byref(ps), begin, end, C.byref(m.c),
                                                        1 if device_only else 0, C.byref(e), C.byref(tm))
        _check(rc, "eg3d_match_polyline_sets")
        if device_only:
            d = {"n_points": int(e.n_points), "n_obs": int(e.n_obs), "n_tasks": int(e.n_tasks),
                 "n_hypotheses": int(e.n_hypotheses), "n_chains": int(e.n_chains), "flags": int(e.flags)}
        else:
            d = D.edgepoints_to_dict(e)
        lib().eg3d_free_edgepoints(C.byref(e))
        d["times"] = {f[0]: getattr(tm, f[0]) for f in D.StageTimes._fields_}
        return d

    def match_polylines_closeness(self, seeds_ptr=None, begin=0, end=None):
        """Pipeline 2's polyline matcher (eg3d_match_polylines_closeness) on seeds [begin, end) of `seeds_ptr`, or of the
        uploaded seeds when it is None (`end` is then required). Returns the accepted reference points, the sets as the
        CSR match_polyline_sets takes (n_sets, row_off, pl_ids), and the call's stats."""
        if end is None:
            if seeds_ptr is None:
                raise Eg3dError("match_polylines_closeness: `end` is required with the uploaded seeds")
            end = int(seeds_ptr.contents.n_seeds) if hasattr(seeds_ptr, "contents") else int(seeds_ptr.n_seeds)
        m, st = D.PolylineMatches(), D.PolymatchStats()
        st.struct_size = C.sizeof(D.PolymatchStats)
        _check(lib().eg3d_match_polylines_closeness(self._h, seeds_ptr, begin, end, C.byref(m), C.byref(st)),
               "eg3d_match_polylines_closeness")
        n_rows = int(m.n_sets) * self.n_views
        row_off = D.as_np(m.row_off, n_rows + 1, np.uint32).copy()
        d = {"refpoints": D.as_np(m.refpoints, int(m.n_refpoints), np.uint32).copy(), "n_sets": int(m.n_sets),
             "row_off": row_off, "pl_ids": D.as_np(m.pl_ids, int(row_off[-1]), np.uint32).copy(),
             "stats": {f[0]: getattr(st, f[0]) for f in D.PolymatchStats._fields_}}
        lib().eg3d_free_polyline_matches(C.byref(m))
        return d

    def similarity_graph(self, seeds_ptr=None, begin=0, end=None):
        """The graph half of pipeline 1's polyline matcher (eg3d_similarity_graph) on seeds [begin, end) of `seeds_ptr`, or
        of the uploaded seeds when it is None (`end` is then required). Returns every array of eg3d_simgraph as numpy
        copies (the weighted adjacency CSR over node ids, the nodes, the point weights, close_polylines and
        close_refpoints) and the call's stats. host.write_compat_graph / host.sets_from_communities take the dict."""
        if end is None:
            if seeds_ptr is None:
                raise Eg3dError("similarity_graph: `end` is required with the uploaded seeds")
            end = int(seeds_ptr.contents.n_seeds) if hasattr(seeds_ptr, "contents") else int(seeds_ptr.n_seeds)
        g, st = D.Simgraph(), D.SimgraphStats()
        st.struct_size = C.sizeof(D.SimgraphStats)
        _check(lib().eg3d_similarity_graph(self._h, seeds_ptr, begin, end, C.byref(g), C.byref(st)), "eg3d_similarity_graph")
        d = D.simgraph_to_dict(g)
        d["stats"] = {f[0]: getattr(st, f[0]) for f in D.SimgraphStats._fields_}
        lib().eg3d_free_simgraph(C.byref(g))
        return d

    def communities(self, g, **params):
        """Pipeline 1's community detection (eg3d_detect_communities) on the weighted adjacency of `g`: a dict with n_nodes,
        adj_off, adj_node and adj_w, such as similarity_graph returns. `params` are the fields of eg3d_louvain_params
        (max_phases, max_sweeps, sweep_threshold, phase_threshold; 0 or absent = the default). Returns ids (int64, numbered by
        ascending smallest member, -1 for a node without a neighbour), n_communities and the call's stats."""
        n = int(g["n_nodes"])
        off = np.ascontiguousarray(g["adj_off"] if n else [0], np.uint32)
        node = np.ascontiguousarray(g["adj_node"] if len(g["adj_node"]) else [0], np.uint32)
        w = np.ascontiguousarray(g["adj_w"] if len(g["adj_w"]) else [0], np.float32)
        if len(off) != n + 1 or (n and (len(g["adj_node"]) != int(off[-1]) or len(g["adj_w"]) != int(off[-1]))):
            raise Eg3dError("communities: adj_off must hold n_nodes + 1 offsets and adj_node / adj_w adj_off[n_nodes] entries")
        sg = D.Simgraph()
        sg.n_nodes = n
        sg.adj_off, sg.adj_node, sg.adj_w = D.np_ptr(off, C.c_uint32), D.np_ptr(node, C.c_uint32), D.np_ptr(w, C.c_float)
        unknown = set(params) - {f[0] for f in D.LouvainParams._fields_[1:]}
        if unknown:
            raise Eg3dError("communities: unknown parameter(s) %s" % sorted(unknown))
        pr = D.LouvainParams(C.sizeof(D.LouvainParams), **params)
        m, st = D.Communities(), D.LouvainStats()
        st.struct_size = C.sizeof(D.LouvainStats)
        _check(lib().eg3d_detect_communities(self._h, C.byref(sg), C.byref(pr), C.byref(m), C.byref(st)), "eg3d_detect_communities")
        d = {"ids": D.as_np(m.ids, int(m.n_nodes), np.int64), "n_communities": int(m.n_communities),
             "stats": {f[0]: getattr(st, f[0]) for f in D.LouvainStats._fields_}}
        lib().eg3d_free_communities(C.byref(m))
        return d

    # ---- include/eg3d_sets_device.h: polyline sets resident on the device, the extractor on item ranges ----
    def upload_polyline_sets(self, n_sets, row_off, pl_ids):
        """eg3d_upload_polyline_sets: a caller's sets made resident and checked on the device. Returns the view
        (DevicePolylineSets), current until the next upload on this context."""
        row_off = np.ascontiguousarray(row_off, np.uint32)
        pl_ids = np.ascontiguousarray(pl_ids if len(pl_ids) else [0], np.uint32)
        ps = D.PolylineSets(n_sets, D.np_ptr(row_off, C.c_uint32), D.np_ptr(pl_ids, C.c_uint32))
        v = D.DevicePolylineSets()
        _check(lib().eg3d_upload_polyline_sets(self._h, C.byref(ps), C.byref(v)), "eg3d_upload_polyline_sets")
        return v

    def polyline_matches_device(self):
        """eg3d_polyline_matches_device: the rows of the last match_polylines_closeness call on this context, in place."""
        v = D.DevicePolylineSets()
        _check(lib().eg3d_polyline_matches_device(self._h, C.byref(v)), "eg3d_polyline_matches_device")
        return v

    def sets_from_communities_device(self, ids=None, n=None, with_stats=False):
        """eg3d_sets_from_communities_device (K13): the sets of a community assignment over the nodes of the last
        similarity_graph call on this context. ids: int64 per node, or None for the ids the last communities call left on
        the device (`n`, the node count, is then required). Returns the view, or (view, stats dict)."""
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.int64)
            n = len(ids) if n is None else n
            keep = ids if len(ids) else np.zeros(1, np.int64)
            p = D.np_ptr(keep, C.c_int64)
        else:
            if n is None:
                raise Eg3dError("sets_from_communities_device: `n` is required with the ids on the device")
            p = None
        v, st = D.DevicePolylineSets(), D.SetsDeviceStats()
        st.struct_size = C.sizeof(D.SetsDeviceStats)
        _check(lib().eg3d_sets_from_communities_device(self._h, p, int(n), C.byref(v), C.byref(st)),
               "eg3d_sets_from_communities_device")
        return (v, {f[0]: getattr(st, f[0]) for f in D.SetsDeviceStats._fields_}) if with_stats else v

    def fetch_polyline_sets(self, view):
        """Test plumbing: (n_sets, row_off, pl_ids) of a device sets view as numpy copies."""
        n_rows = int(view.n_sets) * int(view.n_views)
        a = np.empty(n_rows + 1, np.uint32)
        b = np.empty(int(view.n_ids), np.uint32)
        for dst, src in ((a, view.row_off), (b, view.pl_ids)):
            if dst.nbytes and _hip().hipMemcpy(dst.ctypes.data, C.c_void_p(src), dst.nbytes, 2) != 0:
                raise Eg3dError("hipMemcpy of the device sets failed")
        return int(view.n_sets), a, b

    def polyline_item_samples(self, view, item_begin=0, item_end=None, matched=None):
        """eg3d_polyline_item_samples: the 20 px samples of every item (entry of pl_ids) of [item_begin, item_end), uint32;
        with `matched` (as in match_polyline_sets) the samples left under those intervals."""
        if item_end is None:
            item_end = int(view.n_ids)
        counts = np.zeros(max(item_end - item_begin, 0), np.uint32)
        m = None
        if matched is not None:
            m = matched if isinstance(matched, D.MatchedIntervalsArrays) else D.MatchedIntervalsArrays(matched)
        keep = counts if len(counts) else np.zeros(1, np.uint32)
        _check(lib().eg3d_polyline_item_samples(self._h, C.byref(view), item_begin, item_end, C.byref(m.c) if m else None,
                                                D.np_ptr(keep, C.c_uint32)), "eg3d_polyline_item_samples")
        return counts

    def match_polyline_items(self, view, item_begin=0, item_end=None, sample_base=0, device_only=False, matched=None):
        """eg3d_match_polyline_items: the extractor on items [item_begin, item_end) of a device sets view; key[0] = the
        sample's index within the range + sample_base. Returns what match_polyline_sets returns, plus "n_units" and "n_redone"
        (units the call cut in two and redid because a 32-bit total wrapped)."""
        if item_end is None:
            item_end = int(view.n_ids)
        call = D.ItemsCall(C.sizeof(D.ItemsCall), item_begin, item_end, sample_base)
        m = None
        if matched is not None:
            m = matched if isinstance(matched, D.MatchedIntervalsArrays) else D.MatchedIntervalsArrays(matched)
        e, tm = D.EdgePoints(), D.StageTimes()
        rc = lib().eg3d_match_polyline_items(self._h, C.byref(view), C.byref(call), C.byref(m.c) if m else None,
                                             1 if device_only else 0, C.byref(e), C.byref(tm))
        _check(rc, "eg3d_match_polyline_items")
        if device_only:
            d = {"n_points": int(e.n_points), "n_obs": int(e.n_obs), "n_tasks": int(e.n_tasks),
                 "n_hypotheses": int(e.n_hypotheses), "n_chains": int(e.n_chains), "flags": int(e.flags)}
        else:
            d = D.edgepoints_to_dict(e)
        lib().eg3d_free_edgepoints(C.byref(e))
        d["times"] = {f[0]: getattr(tm, f[0]) for f in D.StageTimes._fields_}
        nu, nr = C.c_uint32(), C.c_uint32()
        _check(lib().eg3d_polyline_items_units(self._h, C.byref(nu), C.byref(nr)), "eg3d_polyline_items_units")
        d["n_units"], d["n_redone"] = int(nu.value), int(nr.value)
        return d

    def last_device_output(self):
        d = D.DeviceEdgePoints()
        _check(lib().eg3d_last_device_output(self._h, C.byref(d)), "eg3d_last_device_output")
        return d

    def fetch_device_output(self):
        """Test/bench plumbing: copies the cloud eg3d_last_device_output views (HBM) into numpy arrays shaped like
        a host result (obs_off gets its final n_obs sentinel). Needs `complete`."""
        d = self.last_device_output()
        if not d.complete:
            raise RuntimeError("the device view does not hold the whole cloud of the last call")

        def fetch(ptr, n, dtype):
            a = np.empty(n, dtype)
            if n and _hip().hipMemcpy(a.ctypes.data, C.cast(ptr, C.c_void_p), a.nbytes, 2) != 0:
                raise RuntimeError("hipMemcpy of the device cloud failed")
            return a
        n, m = int(d.n_points), int(d.n_obs)
        return {"n_points": n, "n_obs": m, "X": fetch(d.X, 3 * n, np.float32).reshape(n, 3),
                "obs_off": np.concatenate([fetch(d.obs_off, n, np.uint64), np.array([m], np.uint64)]),
                "key": fetch(d.key, 4 * n, np.uint32).reshape(n, 4), "obs_view": fetch(d.obs_view, m, np.int32),
                "obs_pl": fetch(d.obs_pl, m, np.uint32), "obs_seg": fetch(d.obs_seg, m, np.uint32),
                "obs_xy": fetch(d.obs_xy, 2 * m, np.float32).reshape(m, 2)}

    def fetch_device_points(self, dev, p0, p1):
        """Test plumbing: points [p0, p1) of a device-resident cloud `dev` (a DeviceEdgePoints: this context's last
        output, or the result of a gather / concat) as numpy arrays, observation offsets rebased to the slice.
        For clouds too large to copy whole (BASELINE config 4 in one call: 82 GB)."""

        def fetch(ptr, first, n, dtype):
            a = np.empty(n, dtype)
            src = C.cast(ptr, C.c_void_p).value + first * a.itemsize if n else 0
            if n and _hip().hipMemcpy(a.ctypes.data, C.c_void_p(src), a.nbytes, 2) != 0:
                raise RuntimeError("hipMemcpy of the device cloud failed")
            return a
        n_all, m_all = int(dev.n_points), int(dev.n_obs)
        n = p1 - p0
        off = fetch(dev.obs_off, p0, n + (1 if p1 < n_all else 0), np.uint64)
        if p1 >= n_all:
            off = np.concatenate([off, np.array([m_all], np.uint64)])
        o0, o1 = (int(off[0]), int(off[-1])) if n else (0, 0)
        m = o1 - o0
        return {"n_points": n, "n_obs": m, "X": fetch(dev.X, 3 * p0, 3 * n, np.float32).reshape(n, 3),
                "obs_off": off - np.uint64(o0), "key": fetch(dev.key, 4 * p0, 4 * n, np.uint32).reshape(n, 4),
                "obs_view": fetch(dev.obs_view, o0, m, np.int32), "obs_pl": fetch(dev.obs_pl, o0, m, np.uint32),
                "obs_seg": fetch(dev.obs_seg, o0, m, np.uint32),
                "obs_xy": fetch(dev.obs_xy, 2 * o0, 2 * m, np.float32).reshape(m, 2)}

    def candidates(self, seeds_ptr, begin, end):
        c = D.Candidates()
        _check(lib().eg3d_candidates_run(self._h, seeds_ptr, begin, end, C.byref(c)), "eg3d_candidates_run")
        d = D.candidates_to_dict(c)
        lib().eg3d_free_candidates(C.byref(c))
        return d

    def polyline_set_candidates(self, n_sets, row_off, pl_ids, begin=0, end=None, matched=None):
        """Stage A of the extractor alone (eg3d_polyline_set_candidates), in task order: the samples that became tasks
        (task_view / task_pl / task_seg / task_xy), the hit lists as a CSR over task * n_views + view (list_off, hit_pl,
        hit_seg, hit_xy; a hit's view is its list's) and n_samples_skipped / n_hits_filtered. `matched` as in
        match_polyline_sets."""
        if end is None:
            end = n_sets
        row_off = np.ascontiguousarray(row_off, np.uint32)
        pl_ids = np.ascontiguousarray(pl_ids if len(pl_ids) else [0], np.uint32)
        ps = D.PolylineSets(n_sets, D.np_ptr(row_off, C.c_uint32), D.np_ptr(pl_ids, C.c_uint32))
        m = None
        if matched is not None:
            m = matched if isinstance(matched, D.MatchedIntervalsArrays) else D.MatchedIntervalsArrays(matched)
        c = D.SetCandidates()
        _check(lib().eg3d_polyline_set_candidates(self._h, C.byref(ps), begin, end, C.byref(m.c) if m else None, C.byref(c)),
               "eg3d_polyline_set_candidates")
        d = D.set_candidates_to_dict(c, self.n_views)
        lib().eg3d_free_set_candidates(C.byref(c))
        return d

    def gn_filter(self, X, obs_off, obs_view, obs_xy, gn_max_mse=2.25, legacy_abs=False):
        X = np.ascontiguousarray(X, np.float32)
        obs_off = np.ascontiguousarray(obs_off, np.uint32)
        obs_view = np.ascontiguousarray(obs_view, np.int32)
        obs_xy = np.ascontiguousarray(obs_xy, np.float32)
        n = len(obs_off) - 1
        Xo = np.zeros((n, 3), np.float32)
        inl = np.zeros(n, np.uint8)
        ms = C.c_float(0)
        _check(lib().eg3d_gn_filter(self._h, D.np_ptr(X, C.c_float), D.np_ptr(obs_off, C.c_uint32),
                                    D.np_ptr(obs_view, C.c_int32), D.np_ptr(obs_xy, C.c_float), n, gn_max_mse,
                                    1 if legacy_abs else 0, D.np_ptr(Xo, C.c_float), D.np_ptr(inl, C.c_uint8),
                                    C.byref(ms)), "eg3d_gn_filter")
        return Xo, inl, ms.value

    # ---- the filter stage on a device-resident cloud (include/eg3d.h) ----
    def device_alloc(self, nbytes):
        """A DeviceArray of nbytes on this context's device."""
        return DeviceArray(nbytes, self.device)

    def upload(self, array):
        """A numpy array copied into a fresh DeviceArray on this context's device."""
        return upload(array, self.device)

    def gn_filter_device(self, cloud, keep=None, gn_max_mse=2.25, legacy_abs=False, X_out=None, inlier=None):
        """eg3d_gn_filter_device on `cloud` (a DeviceEdgePoints). keep / X_out / inlier: DeviceArray or device address;
        X_out and inlier are allocated when not given. Returns (X_out, inlier, hist[n_views + 1] int64, n_inliers, ms);
        n_inliers counts the inliers of no bin (more observations than views) too."""
        n = int(cloud.n_points)
        X_out = X_out if X_out is not None else DeviceArray(12 * n, self.device)
        inlier = inlier if inlier is not None else DeviceArray(n, self.device)
        hist = np.zeros(self.n_views + 1, np.uint64)
        ms, n_inl = C.c_float(0), C.c_uint64(0)
        _check(lib().eg3d_gn_filter_device(self._h, C.byref(cloud), _dev_ptr(keep), gn_max_mse, 1 if legacy_abs else 0,
                                           _dev_ptr(X_out), _dev_ptr(inlier), D.np_ptr(hist, C.c_uint64), C.byref(n_inl),
                                           C.byref(ms)), "eg3d_gn_filter_device")
        return X_out, inlier, hist.astype(np.int64), int(n_inl.value), ms.value

    def compact_device(self, cloud, keep=None, X_new=None, min_obs=-1):
        """eg3d_compact_device: the DeviceEdgePoints of the survivors (buffers of this context, valid until its next
        compaction)."""
        out = D.DeviceEdgePoints()
        _check(lib().eg3d_compact_device(self._h, C.byref(cloud), _dev_ptr(keep), _dev_ptr(X_new), int(min_obs),
                                         C.byref(out)), "eg3d_compact_device")
        return out

    # ---- FP64 triangulation of caller-supplied tracks, K14 (include/eg3d_triangulate.h) ----
    @staticmethod
    def _tri_stats(st):
        return {f[0]: getattr(st, f[0]) for f in D.TriStats._fields_ if f[0] != "struct_size"}

    def triangulate(self, obs_off, obs_view, obs_xy, X0=None, mode=None, with_flags=True):
        """eg3d_triangulate on host arrays (obs_off [n + 1] uint32, obs_view, obs_xy [m, 2]). mode: TRI_FROM_SCRATCH
        (compute_3d_point_coords: DLT, then Gauss-Newton) or TRI_REFINE (Gauss-Newton from X0 [n, 3]); by default REFINE when
        X0 is given. Returns (X [n, 3] float32, valid [n] uint8, flags [n] uint8 or None, stats dict)."""
        if mode is None:
            mode = TRI_FROM_SCRATCH if X0 is None else TRI_REFINE
        obs_off = np.ascontiguousarray(obs_off, np.uint32)
        obs_view = np.ascontiguousarray(obs_view, np.int32)
        obs_xy = np.ascontiguousarray(obs_xy, np.float32)
        n = len(obs_off) - 1
        x0 = None if X0 is None else np.ascontiguousarray(X0, np.float32)
        X, valid = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
        flags = np.zeros(n, np.uint8) if with_flags else None
        st = D.TriStats(struct_size=C.sizeof(D.TriStats))
        _check(lib().eg3d_triangulate(self._h, int(mode), n, D.np_ptr(obs_off, C.c_uint32), D.np_ptr(obs_view, C.c_int32),
                                      D.np_ptr(obs_xy, C.c_float), None if x0 is None else D.np_ptr(x0, C.c_float),
                                      D.np_ptr(X, C.c_float), D.np_ptr(valid, C.c_uint8),
                                      None if flags is None else D.np_ptr(flags, C.c_uint8), C.byref(st)), "eg3d_triangulate")
        return X, valid, flags, self._tri_stats(st)

    def triangulate_device(self, cloud=None, mode=1, X_out=None, valid=None, flags=None, with_flags=True):
        """eg3d_triangulate_device on `cloud` (a DeviceEdgePoints; None = this context's last device output). X_out / valid /
        flags: DeviceArray or device address, allocated when not given (flags only with with_flags); X_out may be the
        cloud's own X. Returns (X_out, valid, flags or None, stats dict); X_out and valid plug into compact_device."""
        n = int((cloud if cloud is not None else self.last_device_output()).n_points)
        X_out = X_out if X_out is not None else DeviceArray(12 * n, self.device)
        valid = valid if valid is not None else DeviceArray(n, self.device)
        if flags is None and with_flags:
            flags = DeviceArray(n, self.device)
        st = D.TriStats(struct_size=C.sizeof(D.TriStats))
        _check(lib().eg3d_triangulate_device(self._h, int(mode), C.byref(cloud) if cloud is not None else None, _dev_ptr(X_out),
                                             _dev_ptr(valid), _dev_ptr(flags), C.byref(st)), "eg3d_triangulate_device")
        return X_out, valid, flags, self._tri_stats(st)

    # ---- the colours of a cloud from the source images, K15 (include/eg3d_colour.h) ----
    @staticmethod
    def _colour_stats(st):
        return {f[0]: getattr(st, f[0]) for f in D.ColourStats._fields_ if f[0] != "struct_size"}

    def upload_images(self, images):
        """eg3d_upload_images: `images` has one entry per view of the rig, an [H, W, 3] uint8 RGB array (each view its own
        size) or None for a view without an image. They stay on this context's device until release_images, the next
        upload or close; a clone does not inherit them."""
        a = D.ImageArgs(images)
        _check(lib().eg3d_upload_images(self._h, *a.args()), "eg3d_upload_images")

    def release_images(self):
        _check(lib().eg3d_release_images(self._h), "eg3d_release_images")

    def colour_device(self, cloud=None, keep=None, rgb=None, flags=None, with_flags=True):
        """eg3d_colour_device on `cloud` (a DeviceEdgePoints; None = this context's last device output). keep / rgb / flags:
        DeviceArray or device address; rgb [n, 3] and flags [n] are allocated when not given (flags only with with_flags).
        Returns (rgb, flags or None, stats dict)."""
        n = int((cloud if cloud is not None else self.last_device_output()).n_points)
        rgb = rgb if rgb is not None else DeviceArray(3 * n, self.device)
        if flags is None and with_flags:
            flags = DeviceArray(n, self.device)
        st = D.ColourStats(struct_size=C.sizeof(D.ColourStats))
        _check(lib().eg3d_colour_device(self._h, C.byref(cloud) if cloud is not None else None, _dev_ptr(keep), _dev_ptr(rgb),
                                        _dev_ptr(flags), C.byref(st)), "eg3d_colour_device")
        return rgb, flags, self._colour_stats(st)

    def colour_points(self, obs_off, obs_view, obs_xy, keep=None):
        """eg3d_colour_points on host arrays (obs_off [n + 1] uint32, obs_view, obs_xy [m, 2], keep [n] uint8 or None).
        Returns (rgb [n, 3] uint8, flags [n] uint8: COLOUR_FLAG_EMPTY, stats dict)."""
        obs_off = np.ascontiguousarray(obs_off, np.uint32)
        obs_view = np.ascontiguousarray(obs_view, np.int32)
        obs_xy = np.ascontiguousarray(obs_xy, np.float32)
        n = len(obs_off) - 1
        k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        rgb, flags = np.zeros((n, 3), np.uint8), np.zeros(n, np.uint8)
        st = D.ColourStats(struct_size=C.sizeof(D.ColourStats))
        _check(lib().eg3d_colour_points(self._h, n, D.np_ptr(obs_off, C.c_uint32), D.np_ptr(obs_view, C.c_int32),
                                        D.np_ptr(obs_xy, C.c_float), None if k is None else D.np_ptr(k, C.c_uint8),
                                        D.np_ptr(rgb, C.c_uint8), D.np_ptr(flags, C.c_uint8), C.byref(st)), "eg3d_colour_points")
        return rgb, flags, self._colour_stats(st)

    # ---- a 4 x 4 transform applied to a cloud's points, K16 (include/eg3d_transform.h) ----
    @staticmethod
    def _transform_stats(st):
        return {f[0]: getattr(st, f[0]) for f in D.TransformStats._fields_ if f[0] not in ("struct_size", "reserved")}

    @staticmethod
    def _T16(T):
        T = np.ascontiguousarray(T, np.float64).reshape(-1)
        if T.size != 16:
            raise ValueError("T must hold 16 values (a row-major 4 x 4)")
        return T

    def transform_device(self, T, keep=None, out=None, cloud=None):
        """eg3d_transform_device: the points of `cloud` (a DeviceEdgePoints; None = this context's last device output)
        through T (row-major 4 x 4, float64; host.similarity_fit). keep: DeviceArray or device address of [n] uint8, None =
        every point; out: where the [n, 3] result goes, None = in place. A DeviceArray whose size is not the cloud's
        (n bytes for keep, 12 n for out) is refused here with ValueError. Returns the stats dict."""
        n = int((cloud if cloud is not None else self.last_device_output()).n_points)
        if isinstance(keep, DeviceArray) and keep.nbytes != n:
            raise ValueError("transform_device: keep holds %d bytes, the cloud %d points" % (keep.nbytes, n))
        if isinstance(out, DeviceArray) and out.nbytes != 12 * n:
            raise ValueError("transform_device: out holds %d bytes, the cloud needs %d" % (out.nbytes, 12 * n))
        T = self._T16(T)
        st = D.TransformStats(struct_size=C.sizeof(D.TransformStats))
        _check(lib().eg3d_transform_device(self._h, C.byref(cloud) if cloud is not None else None, D.np_ptr(T, C.c_double),
                                           _dev_ptr(keep), _dev_ptr(out), C.byref(st)), "eg3d_transform_device")
        return self._transform_stats(st)

    def transform_points(self, T, X):
        """eg3d_transform_points on a host array X [n, 3] float32. Returns (X' [n, 3] float32, stats dict)."""
        T = self._T16(T)
        X = np.ascontiguousarray(X, np.float32).reshape(-1, 3)
        out = np.empty_like(X)
        st = D.TransformStats(struct_size=C.sizeof(D.TransformStats))
        _check(lib().eg3d_transform_points(self._h, D.np_ptr(T, C.c_double), D.np_ptr(X, C.c_float), len(X),
                                           D.np_ptr(out, C.c_float), C.byref(st)), "eg3d_transform_points")
        return out, self._transform_stats(st)

    def filter_resident(self, gn_max_mse=2.25, legacy_abs=False, forced_min_filter=-1, base_hist=None, to_host=True):
        """eg3d_filter_resident on the last device output. Returns (cloud dict or None, DeviceEdgePoints, stats dict)."""
        e, dv, st = D.EdgePoints(), D.DeviceEdgePoints(), D.FilterStats()
        st.struct_size = C.sizeof(D.FilterStats)
        bh = None
        if base_hist is not None:
            bh = np.ascontiguousarray(base_hist, np.uint64)
            if len(bh) != self.n_views + 1:
                raise ValueError("base_hist needs n_views + 1 entries")
        _check(lib().eg3d_filter_resident(self._h, gn_max_mse, 1 if legacy_abs else 0, int(forced_min_filter),
                                          D.np_ptr(bh, C.c_uint64) if bh is not None else None, 1 if to_host else 0,
                                          C.byref(e) if to_host else None, C.byref(dv), C.byref(st)), "eg3d_filter_resident")
        d = None
        if to_host:
            d = D.edgepoints_to_dict(e)
            lib().eg3d_free_edgepoints(C.byref(e))
        return d, dv, {f[0]: getattr(st, f[0]) for f in D.FilterStats._fields_}

    # ---- the 3 px dedup on a device-resident cloud (include/eg3d.h) ----
    def dedup_device(self, cloud, index_base=0, reset=True, keep=None):
        """eg3d_dedup_device on `cloud` (a DeviceEdgePoints): the mask by the first-claim rule (cloudnp.np_dedup) against
        this context's claim map. reset: clear the map first; otherwise the claims of the earlier calls stand and this
        cloud's points count from index_base. keep: DeviceArray or device address of n_points bytes, allocated when not
        given. Returns (keep, n_kept)."""
        n = int(cloud.n_points)
        keep = keep if keep is not None else DeviceArray(n, self.device)
        n_kept = C.c_uint64(0)
        _check(lib().eg3d_dedup_device(self._h, C.byref(cloud), int(index_base), 1 if reset else 0, _dev_ptr(keep),
                                       C.byref(n_kept)), "eg3d_dedup_device")
        return keep, int(n_kept.value)

    def dedup_resident(self, index_base=0, reset=True, with_filter=False, gn_max_mse=2.25, legacy_abs=False,
                       forced_min_filter=-1, base_hist=None, to_host=True):
        """eg3d_dedup_resident on the last device output: dedup, optionally the Gauss-Newton filter and the observation
        threshold, compaction, optionally the copy of the survivors. Returns (cloud dict or None, DeviceEdgePoints, stats
        dict)."""
        e, dv, st = D.EdgePoints(), D.DeviceEdgePoints(), D.DedupStats()
        st.struct_size = C.sizeof(D.DedupStats)
        bh = None
        if base_hist is not None:
            bh = np.ascontiguousarray(base_hist, np.uint64)
            if len(bh) != self.n_views + 1:
                raise ValueError("base_hist needs n_views + 1 entries")
        _check(lib().eg3d_dedup_resident(self._h, int(index_base), 1 if reset else 0, 1 if with_filter else 0, gn_max_mse,
                                         1 if legacy_abs else 0, int(forced_min_filter),
                                         D.np_ptr(bh, C.c_uint64) if bh is not None else None, 1 if to_host else 0,
                                         C.byref(e) if to_host else None, C.byref(dv), C.byref(st)), "eg3d_dedup_resident")
        d = None
        if to_host:
            d = D.edgepoints_to_dict(e)
            lib().eg3d_free_edgepoints(C.byref(e))
        return d, dv, {f[0]: getattr(st, f[0]) for f in D.DedupStats._fields_}

    # ---- the dedup in phases (include/eg3d_dedup_phases.h): claim in any order, merge claim maps, then keep ----
    def dedup_claim(self, cloud, index_base=0, reset=False):
        """eg3d_dedup_claim: the claim pass alone on `cloud` (a DeviceEdgePoints), its points counting from index_base within
        the run. Clouds may be claimed in any order and on any context; reset empties this context's map first. A cloud
        whose offsets do not ascend is refused and leaves the map as it was."""
        _check(lib().eg3d_dedup_claim(self._h, C.byref(cloud), int(index_base), 1 if reset else 0), "eg3d_dedup_claim")

    def dedup_keep(self, cloud, index_base=0, keep=None):
        """eg3d_dedup_keep: the keep pass alone, against this context's map as it stands (its own claims and whatever was
        merged or reduced into it). keep: DeviceArray or device address of n_points bytes, allocated when not given.
        Returns (keep, n_kept). Refused while the context holds no valid map."""
        n = int(cloud.n_points)
        keep = keep if keep is not None else DeviceArray(n, self.device)
        n_kept = C.c_uint64(0)
        _check(lib().eg3d_dedup_keep(self._h, C.byref(cloud), int(index_base), _dev_ptr(keep), C.byref(n_kept)),
               "eg3d_dedup_keep")
        return keep, int(n_kept.value)

    def dedup_claims(self):
        """eg3d_dedup_claims: (device address, n_cells) of this context's claim map, created empty (0xFFFFFFFF) when there
        is no valid one. Borrowed: valid until the context is closed or a dedup call on it fails. A caller may lower
        entries in place (a min all-reduce does); the map then holds those claims too."""
        p, n = C.c_void_p(), C.c_uint64(0)
        _check(lib().eg3d_dedup_claims(self._h, C.byref(p), C.byref(n)), "eg3d_dedup_claims")
        return int(p.value), int(n.value)

    def fetch_dedup_claims(self):
        """Test/bench plumbing: a host copy of the claim map (uint32[n_cells])."""
        p, n = self.dedup_claims()
        a = np.empty(n, np.uint32)
        if n and _hip().hipMemcpy(a.ctypes.data, C.c_void_p(p), a.nbytes, 2) != 0:
            raise Eg3dError("hipMemcpy from the device failed")
        return a

    def dedup_merge_claims(self, other, n_cells=None):
        """eg3d_dedup_merge_claims: this context's map becomes the element-wise minimum of itself and `other` — another
        Context (its map), or (DeviceArray or device address, n_cells) of any device-readable uint32 array, 4-byte aligned.
        Returns the number of entries that got smaller."""
        if isinstance(other, Context):
            other, n_cells = other.dedup_claims()
        if n_cells is None:
            raise ValueError("n_cells is needed with a device address")
        n_low = C.c_uint64(0)
        _check(lib().eg3d_dedup_merge_claims(self._h, _dev_ptr(other), int(n_cells), C.byref(n_low)), "eg3d_dedup_merge_claims")
        return int(n_low.value)

    def dedup_phase_ms(self):
        """eg3d_dedup_phase_ms: device time of the last dedup_claim / dedup_keep / dedup_merge_claims of this context."""
        ms = C.c_float(0)
        _check(lib().eg3d_dedup_phase_ms(self._h, C.byref(ms)), "eg3d_dedup_phase_ms")
        return ms.value

    # ---- the PLGMatchesManager replay on a device-resident cloud (include/eg3d.h) ----
    def replay_device(self, cloud=None, to_host=True):
        """eg3d_replay_device on `cloud` (a DeviceEdgePoints; None = the last device output): the 3-D polyline graph and
        the matched 2-D intervals of row a17. Returns (graph or None, DeviceGraph3D, stats dict); the graph is a dict of
        numpy arrays under the field names of eg3d_graph3d, as host.replay_matches returns it; the DeviceGraph3D views
        buffers of this context that stay valid until its next replay."""
        g, dv, st = D.Graph3D(), D.DeviceGraph3D(), D.ReplayStats()
        st.struct_size = C.sizeof(D.ReplayStats)
        _check(lib().eg3d_replay_device(self._h, C.byref(cloud) if cloud is not None else None, C.byref(dv),
                                        C.byref(g) if to_host else None, C.byref(st)), "eg3d_replay_device")
        d = None
        if to_host:
            d = D.graph3d_to_dict(g)
            lib().eg3d_free_graph3d(C.byref(g))
        return d, dv, {f[0]: getattr(st, f[0]) for f in D.ReplayStats._fields_}

    # ---- the replay that accumulates over the calls of a run (include/eg3d_accumulate.h) ----
    def replay_accumulate(self, cloud=None, reset=False, to_host=True, materialise=True):
        """eg3d_replay_accumulate: add `cloud` (a DeviceEdgePoints; None = the last device output) to this context's
        accumulator; reset starts a new graph with it. Returns (graph or None, DeviceGraph3D or None, stats dict). The
        graph is that of all clouds added so far, as host.replay_matches builds it from their concatenation;
        materialise=False only adds the claims (both None). The DeviceGraph3D views buffers of the accumulator that stay
        valid until the next replay_accumulate on this context."""
        g, dv, st = D.Graph3D(), D.DeviceGraph3D(), D.ReplayStats()
        st.struct_size = C.sizeof(D.ReplayStats)
        to_host = to_host and materialise
        _check(lib().eg3d_replay_accumulate(self._h, C.byref(cloud) if cloud is not None else None, 1 if reset else 0,
                                            C.byref(dv) if materialise else None, C.byref(g) if to_host else None,
                                            C.byref(st)), "eg3d_replay_accumulate")
        d = None
        if to_host:
            d = D.graph3d_to_dict(g)
            lib().eg3d_free_graph3d(C.byref(g))
        return d, (dv if materialise else None), {f[0]: getattr(st, f[0]) for f in D.ReplayStats._fields_}

    def replay_accumulated(self):
        """eg3d_replay_accumulated: {"n_points", "n_pairs", "state_bytes"} of the accumulator; n_points is the index_base
        of the next cloud of the run for dedup_device."""
        n, p, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().eg3d_replay_accumulated(self._h, C.byref(n), C.byref(p), C.byref(b)), "eg3d_replay_accumulated")
        return {"n_points": int(n.value), "n_pairs": int(p.value), "state_bytes": int(b.value)}

    # ---- the accumulator takes the graph of the run that follows (include/eg3d_replay_merge.h) ----
    def upload_graph(self, graph):
        """A graph dict (as replay_device or host.replay_matches return it) as caller-built device arrays:
        (DeviceGraph3D, the DeviceArrays that own the memory — keep them for as long as the view is used)."""
        dv, held = D.DeviceGraph3D(), {}
        dv.n_nodes, dv.n_real_nodes, dv.n_polylines = int(graph["n_nodes"]), int(graph["n_real_nodes"]), int(graph["n_polylines"])
        dv.n_scene_polylines = int(graph.get("n_scene_polylines", len(graph["iv_off"]) - 1))
        flat = {k: np.ascontiguousarray(graph[k], t).reshape(-1) for k, t in D.GRAPH3D_ARRAYS}
        D.graph3d_lengths_check(graph, flat)
        for k, t in D.GRAPH3D_ARRAYS:
            a = flat[k]
            held[k] = self.upload(a if a.size else np.zeros(1, t))
            setattr(dv, k, held[k].ptr)
        return dv, held

    def replay_merge(self, later, n_points, n_pairs=0, reset=False, to_host=True, materialise=True):
        """eg3d_replay_merge_graph: this context's accumulator takes, in place of the cloud of the run that follows
        directly, the graph a replay of it built elsewhere. `later`: a DeviceGraph3D of ANOTHER context on this device
        (replay_device / replay_accumulate / replay_merge), or a graph dict, which is uploaded. n_points: the points of
        later's cloud; n_pairs: its pairs, only added to the totals. Returns what replay_accumulate returns."""
        held = None
        if not isinstance(later, D.DeviceGraph3D):
            later, held = self.upload_graph(later)
        g, dv, st = D.Graph3D(), D.DeviceGraph3D(), D.ReplayStats()
        st.struct_size = C.sizeof(D.ReplayStats)
        to_host = to_host and materialise
        _check(lib().eg3d_replay_merge_graph(self._h, C.byref(later), int(n_points), int(n_pairs), 1 if reset else 0,
                                             C.byref(dv) if materialise else None, C.byref(g) if to_host else None,
                                             C.byref(st)), "eg3d_replay_merge_graph")
        del held
        d = None
        if to_host:
            d = D.graph3d_to_dict(g)
            lib().eg3d_free_graph3d(C.byref(g))
        return d, (dv if materialise else None), {f[0]: getattr(st, f[0]) for f in D.ReplayStats._fields_}

    # ---- the 3-D edge model of a graph3d (include/eg3d/edges.h, K17) ----
    def _edge_chains(self, call, what, max_dist, simplify, to_host):
        ch, dv, st = D.EdgeChains(), D.DeviceEdgeChains(), D.EdgesStats()
        st.struct_size = C.sizeof(D.EdgesStats)
        _check(call(float(max_dist), 1 if simplify else 0, C.byref(dv), C.byref(ch) if to_host else None, C.byref(st)), what)
        if not to_host:
            return {"device": dv, "stats": D.edge_chains_to_dict(D.EdgeChains(), st)["stats"]}
        d = D.edge_chains_to_dict(ch, st)
        lib().eg3d_free_edge_chains(C.byref(ch))
        d["device"] = dv
        return d

    def edge_chains_device(self, graph=None, max_dist=0.01, simplify=True, to_host=True):
        """eg3d_edge_chains_device on `graph` (a DeviceGraph3D on this context's device; None = the result of this context's
        last replay_device): the graph's polylines traced into maximal chains, simplified with the reference's
        simplify_polyline at tolerance max_dist (scene units) and measured, on the device. Returns a dict of numpy arrays —
        chain_off, chain_node, flags, s_off, s_node, length — with "stats" and "device" (the DeviceEdgeChains, buffers of
        this context valid until its next edge-chains call); to_host=False leaves the arrays out."""
        L = lib()
        return self._edge_chains(lambda *a: L.eg3d_edge_chains_device(self._h, C.byref(graph) if graph is not None else None, *a),
                                 "eg3d_edge_chains_device", max_dist, simplify, to_host)

    def edge_chains(self, graph, max_dist=0.01, simplify=True, to_host=True):
        """eg3d_edge_chains: the same on a host graph (a dict as replay_device or host.replay_matches return it; only n_nodes,
        n_polylines, node_X, pl_start, pl_end, conn_off and conn_pl are read), uploaded for the call."""
        ga, L = D.EdgesGraphArrays(graph), lib()
        return self._edge_chains(lambda *a: L.eg3d_edge_chains(self._h, C.byref(ga.c), *a), "eg3d_edge_chains", max_dist, simplify,
                                 to_host)

    # ---- cloud-to-cloud nearest distances (include/eg3d/nearest.hpp, K18) ----
    def cloud_index(self, X=None, cloud=None, keep=None, cell=None):
        """A CloudIndex over a reference point set: X, a host array [n, 3] (eg3d_cloud_index_build; keep: a host array [n]
        or None), or — X is None — `cloud`, a DeviceEdgePoints on this context's device, None = this context's last device
        output (eg3d_cloud_index_build_device; keep: DeviceArray or device address of [n] uint8, or None). cell: the grid's
        edge, the largest max_dist a query may ask for. Free the index (close(), or `with`) before the context is closed."""
        if cell is None:
            raise ValueError("cloud_index: cell is required")
        h, st = C.c_void_p(), D.CloudIndexStats(struct_size=C.sizeof(D.CloudIndexStats))
        if X is not None:
            if cloud is not None:
                raise ValueError("cloud_index: X or cloud, not both")
            X = np.ascontiguousarray(X, np.float32).reshape(-1, 3)
            k = None if keep is None else np.ascontiguousarray(keep, np.uint8).reshape(-1)
            if k is not None and len(k) != len(X):
                raise ValueError("cloud_index: X and keep differ in length")
            _check(lib().eg3d_cloud_index_build(self._h, D.np_ptr(X, C.c_float) if len(X) else None, len(X),
                                                D.np_ptr(k, C.c_uint8) if k is not None and len(X) else None, float(cell),
                                                C.byref(h), C.byref(st)), "eg3d_cloud_index_build")
        else:
            n = int((cloud if cloud is not None else self.last_device_output()).n_points)
            if isinstance(keep, DeviceArray) and keep.nbytes != n:
                raise ValueError("cloud_index: keep holds %d bytes, the cloud %d points" % (keep.nbytes, n))
            _check(lib().eg3d_cloud_index_build_device(self._h, C.byref(cloud) if cloud is not None else None, _dev_ptr(keep),
                                                       float(cell), C.byref(h), C.byref(st)), "eg3d_cloud_index_build_device")
        return CloudIndex(self, h, D.cloud_index_stats_to_dict(st))

    def nearest_device(self, index, max_dist, cloud=None, keep=None, thresholds=(), to_host=True, d2=None, nn=None):
        """eg3d_cloud_nearest_device: every point of `cloud` (None = this context's last device output) against `index`.
        keep, d2 ([n] float32), nn ([n] uint32): DeviceArray or device address; d2 and nn are allocated when not given. A
        DeviceArray of another size than the cloud's is refused here with ValueError. Returns a dict: "d2_dev", "nn_dev"
        (the device arrays), "stats" (the figures, with mean and median as distances) and, with to_host, "d2" and "nn" as
        numpy arrays."""
        n = int((cloud if cloud is not None else self.last_device_output()).n_points)
        for name, a, size in (("keep", keep, n), ("d2", d2, 4 * n), ("nn", nn, 4 * n)):
            if isinstance(a, DeviceArray) and a.nbytes != size:
                raise ValueError("nearest_device: %s holds %d bytes, the cloud needs %d" % (name, a.nbytes, size))
        d2 = d2 if d2 is not None else DeviceArray(4 * n, self.device)
        nn = nn if nn is not None else DeviceArray(4 * n, self.device)
        st = D.nearest_stats_new(thresholds)
        _check(lib().eg3d_cloud_nearest_device(self._h, C.byref(cloud) if cloud is not None else None, _dev_ptr(keep), index._h,
                                               float(max_dist), _dev_ptr(d2), _dev_ptr(nn), C.byref(st)), "eg3d_cloud_nearest_device")
        out = {"d2_dev": d2, "nn_dev": nn, "stats": D.nearest_stats_to_dict(st, max_dist)}
        if to_host:
            if not (isinstance(d2, DeviceArray) and isinstance(nn, DeviceArray)):
                raise ValueError("nearest_device: to_host needs d2 and nn as DeviceArray")
            out["d2"], out["nn"] = d2.numpy(np.float32), nn.numpy(np.uint32)
        return out

    def nearest_points(self, index, X, max_dist, keep=None, thresholds=()):
        """eg3d_cloud_nearest_points: the host array X [n, 3] against `index`. Returns (d2 [n] float32, nn [n] uint32, stats
        dict) — bit for bit what host.cloud_nearest returns."""
        X = np.ascontiguousarray(X, np.float32).reshape(-1, 3)
        k = None if keep is None else np.ascontiguousarray(keep, np.uint8).reshape(-1)
        if k is not None and len(k) != len(X):
            raise ValueError("nearest_points: X and keep differ in length")
        n = len(X)
        d2, nn = np.empty(n, np.float32), np.empty(n, np.uint32)
        st = D.nearest_stats_new(thresholds)
        _check(lib().eg3d_cloud_nearest_points(self._h, D.np_ptr(X, C.c_float) if n else None, n,
                                               D.np_ptr(k, C.c_uint8) if k is not None and n else None, index._h, float(max_dist),
                                               D.np_ptr(d2, C.c_float) if n else None, D.np_ptr(nn, C.c_uint32) if n else None,
                                               C.byref(st)), "eg3d_cloud_nearest_points")
        return d2, nn, D.nearest_stats_to_dict(st, max_dist)

    def compare_clouds(self, ref_X, max_dist, thresholds=(), cloud=None, keep=None, ref_keep=None):
        """Both directions of a comparison of a resident cloud (None = the last device output; keep: device mask) with the
        host array ref_X [m, 3] (ref_keep: host mask), the cell being max_dist: {"accuracy": the cloud's points against an
        index over ref_X, "completeness": ref_X against an index over the cloud}, each a figures dict with `mean` and
        `median` as distances — what host.compare_clouds gives on the fetched cloud."""
        with self.cloud_index(X=ref_X, keep=ref_keep, cell=max_dist) as ref_index:
            acc = self.nearest_device(ref_index, max_dist, cloud=cloud, keep=keep, thresholds=thresholds, to_host=False)["stats"]
        with self.cloud_index(cloud=cloud, keep=keep, cell=max_dist) as own_index:
            comp = self.nearest_points(own_index, ref_X, max_dist, keep=ref_keep, thresholds=thresholds)[2]
        return {"accuracy": acc, "completeness": comp}

    def fetch_device_graph(self, dv):
        """Test/bench plumbing: the graph a DeviceGraph3D views (HBM), copied into the dict graph3d_to_dict gives."""
        def fetch(ptr, n, dtype):
            a = np.empty(int(n), dtype)
            if a.nbytes and _hip().hipMemcpy(a.ctypes.data, C.c_void_p(ptr), a.nbytes, 2) != 0:
                raise Eg3dError("hipMemcpy of the device graph failed")
            return a
        nn, npl, nsp = int(dv.n_nodes), int(dv.n_polylines), int(dv.n_scene_polylines)
        conn_off = fetch(dv.conn_off, nn + 1, np.uint64)
        iv_off = fetch(dv.iv_off, nsp + 1, np.uint64)
        nc, ni = int(conn_off[-1]), int(iv_off[-1])
        return {"n_nodes": nn, "n_real_nodes": int(dv.n_real_nodes), "n_polylines": npl,
                "node_X": fetch(dv.node_X, 3 * nn, np.float32).reshape(nn, 3), "node_point": fetch(dv.node_point, nn, np.uint64),
                "pl_start": fetch(dv.pl_start, npl, np.uint32), "pl_end": fetch(dv.pl_end, npl, np.uint32),
                "conn_off": conn_off, "conn_pl": fetch(dv.conn_pl, nc, np.uint32), "iv_off": iv_off,
                "iv_start_seg": fetch(dv.iv_start_seg, ni, np.uint32),
                "iv_start_xy": fetch(dv.iv_start_xy, 2 * ni, np.float32).reshape(ni, 2),
                "iv_end_seg": fetch(dv.iv_end_seg, ni, np.uint32),
                "iv_end_xy": fetch(dv.iv_end_xy, 2 * ni, np.float32).reshape(ni, 2)}
