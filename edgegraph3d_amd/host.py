"""Python view of libeg3d_host.so: synthetic workloads, grid builder, host post steps."""
import ctypes as C
import os

import numpy as np

from . import _cdefs as D
from ._cabi import bind_library

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libeg3d_host.so")
        if not os.path.exists(path):
            raise RuntimeError("libeg3d_host.so is not built: run `python -m edgegraph3d_amd.build`")
        _LIB = bind_library(C.CDLL(path), "host")
    return _LIB


def default_config(index):
    c = D.SynthConfig()
    lib().eg3d_synth_default_config(C.byref(c), index)
    return c


class Synth:
    """Seeded synthetic scene + seeds (owned by the native library)."""

    def __init__(self, config):
        if isinstance(config, int):
            config = default_config(config)
        self.config = config
        self._h = lib().eg3d_synth_create(C.byref(config))
        if not self._h:
            raise RuntimeError("eg3d_synth_create failed")
        self.scene = lib().eg3d_synth_scene(self._h)   # POINTER(Scene)
        self.seeds = lib().eg3d_synth_seeds(self._h)   # POINTER(Seeds)

    def close(self):
        if self._h:
            lib().eg3d_synth_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_views(self):
        return int(self.scene.contents.n_views)

    @property
    def n_seeds(self):
        return int(self.seeds.contents.n_seeds)

    @property
    def total_segments(self):
        return int(lib().eg3d_synth_total_segments(self._h))

    def seeds_np(self):
        s = self.seeds.contents
        n = int(s.n_seeds)
        off = D.as_np(s.trk_off, n + 1, np.uint32)
        m = int(off[-1])
        return off, D.as_np(s.trk_view, m, np.int32), D.as_np(s.trk_xy, 2 * m, np.float32).reshape(m, 2)

    def seed_truth(self):
        """[n_seeds, 3] noise-free 3-D positions the seeds were generated from"""
        return D.as_np(lib().eg3d_synth_seed_truth(self._h), 3 * self.n_seeds, np.float32).reshape(-1, 3).astype(np.float64)

    def scene_np(self):
        s = self.scene.contents
        V = int(s.n_views)
        vpo = D.as_np(s.view_pl_off, V + 1, np.uint32)
        NP = int(vpo[-1])
        pvo = D.as_np(s.pl_vtx_off, NP + 1, np.uint32)
        NV = int(pvo[-1])
        return {
            "n_views": V, "width": int(s.width), "height": int(s.height),
            "cam_P": D.as_np(s.cam_P, V * 16, np.float32).reshape(V, 16),
            "F": D.as_np(s.F, V * V * 9, np.float64).reshape(V, V, 9),
            "F_valid": D.as_np(s.F_valid, V * V, np.uint8).reshape(V, V),
            "view_pl_off": vpo, "pl_vtx_off": pvo,
            "vtx_xy": D.as_np(s.vtx_xy, 2 * NV, np.float32).reshape(NV, 2),
            "pl_start": D.as_np(s.pl_start, NP, np.uint32), "pl_end": D.as_np(s.pl_end, NP, np.uint32),
            "pl_valid": D.as_np(s.pl_valid, NP, np.uint8),
        }

    def polyline_sets(self, max_sets=None):
        """Synthetic "potentially compatible polylines" sets (the input of pipelines 1-2, produced in
        the reference by the polyline matcher): one set per 3-D curve = the valid polylines of every
        view generated from it. Returns (n_sets, row_off[n_sets*V+1], pl_ids) — a CSR over rows
        (set * V + view), view-local polyline ids ascending per row."""
        sc = self.scene_np()
        V, vpo = sc["n_views"], sc["view_pl_off"]
        NP = int(vpo[-1])
        curve = D.as_np(lib().eg3d_synth_polyline_curve(self._h), NP, np.uint32)
        n_sets = int(lib().eg3d_synth_n_curves(self._h))
        if max_sets is not None:
            n_sets = min(n_sets, max_sets)
        nvtx = np.diff(sc["pl_vtx_off"])
        row_off, ids = [0], []
        for c in range(n_sets):
            for v in range(V):
                a, b = int(vpo[v]), int(vpo[v + 1])
                sel = np.nonzero((curve[a:b] == c) & (sc["pl_valid"][a:b] != 0) & (nvtx[a:b] >= 2))[0]
                ids.extend(int(i) for i in sel)
                row_off.append(len(ids))
        return n_sets, np.asarray(row_off, np.uint32), np.asarray(ids if ids else [0], np.uint32)[:len(ids)]

    def points(self, n_points, rng_seed=0xC5):
        """Config-5 workload: returns X, obs_off, obs_view, obs_xy (numpy copies)."""
        X, off, view, xy = D.f32p(), D.u32p(), D.i32p(), D.f32p()
        rc = lib().eg3d_synth_points(self._h, n_points, rng_seed, C.byref(X), C.byref(off), C.byref(view), C.byref(xy))
        if rc != 0:
            raise RuntimeError("eg3d_synth_points failed")
        o = D.as_np(off, n_points + 1, np.uint32)
        m = int(o[-1])
        out = (D.as_np(X, 3 * n_points, np.float32).reshape(n_points, 3), o, D.as_np(view, m, np.int32),
               D.as_np(xy, 2 * m, np.float32).reshape(m, 2))
        for p in (X, off, view, xy):
            lib().eg3d_host_free(p)
        return out


def replay_matches(scene_ptr, cloud):
    """Row a17: the 3-D polyline graph and matched 2-D intervals PLGMatchesManager would hold after
    the path emitted `cloud` (a dict as returned by Context.match_refpoints)."""
    ep = D.EdgePointsArrays(cloud)
    g = D.Graph3D()
    rc = lib().eg3d_host_replay_matches(scene_ptr, C.byref(ep.c), C.byref(g))
    if rc != 0:
        raise RuntimeError("eg3d_host_replay_matches failed (%d)" % rc)
    d = D.graph3d_to_dict(g)
    lib().eg3d_host_free_graph3d(C.byref(g))
    return d


class ReplayState:
    """The matches manager as an object that lives through a run (include/eg3d_host_accumulate.h): add(cloud) the clouds
    of the run in order; graph() is at any time what replay_matches builds from their concatenation. `scene_ptr` is
    borrowed: keep its owner for as long as the state."""

    def __init__(self, scene_ptr):
        self._h = lib().eg3d_host_replay_state_create(scene_ptr)
        if not self._h:
            raise RuntimeError("eg3d_host_replay_state_create failed")

    def add(self, cloud):
        """Raises ValueError when the cloud is refused (the state is then as it was)."""
        ep = D.EdgePointsArrays(cloud)
        rc = lib().eg3d_host_replay_state_add(self._h, C.byref(ep.c))
        if rc != 0:
            raise ValueError("eg3d_host_replay_state_add refused the cloud (%d)" % rc)

    def merge(self, graph, n_points):
        """eg3d_host_replay_state_merge_graph (include/eg3d_host_replay_merge.h): in place of the cloud of the run that
        follows directly, the graph a replay of it built elsewhere (a dict as graph() returns it) and the number of its
        points. Raises ValueError when the graph is refused (the state is then as it was); .code holds the C code."""
        ga = D.Graph3DArrays(graph)
        rc = lib().eg3d_host_replay_state_merge_graph(self._h, C.byref(ga.c), int(n_points))
        if rc != 0:
            err = ValueError("eg3d_host_replay_state_merge_graph refused the graph (%d)" % rc)
            err.code = rc
            raise err

    def graph(self):
        g = D.Graph3D()
        rc = lib().eg3d_host_replay_state_graph(self._h, C.byref(g))
        if rc != 0:
            raise RuntimeError("eg3d_host_replay_state_graph failed (%d)" % rc)
        d = D.graph3d_to_dict(g)
        lib().eg3d_host_free_graph3d(C.byref(g))
        return d

    @property
    def n_points(self):
        return int(lib().eg3d_host_replay_state_points(self._h))

    def close(self):
        if self._h:
            lib().eg3d_host_replay_state_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the 3 px dedup in phases on host clouds (include/eg3d_host_dedup_phases.h) ----
def dedup_empty_claims(n_views, width, height):
    """An empty claim map: uint32[eg3d_host_dedup_n_cells] of 0xFFFFFFFF."""
    return np.full(int(lib().eg3d_host_dedup_n_cells(n_views, width, height)), 0xFFFFFFFF, np.uint32)


def dedup_claim(cloud, n_views, width, height, first, index_base=0):
    """eg3d_host_dedup_claim of a cloud dict into the map `first` (contiguous uint32, lowered in place). Raises ValueError
    when the cloud is refused (the map is then as it was)."""
    ep = D.EdgePointsArrays(cloud)
    if first.dtype != np.uint32 or not first.flags["C_CONTIGUOUS"] or first.size != lib().eg3d_host_dedup_n_cells(n_views, width, height):
        raise ValueError("first must be a contiguous uint32 map of this rig")
    rc = lib().eg3d_host_dedup_claim(n_views, width, height, C.byref(ep.c), int(index_base), D.np_ptr(first, C.c_uint32))
    if rc != 0:
        raise ValueError("eg3d_host_dedup_claim refused the cloud (%d)" % rc)
    return first


def dedup_keep(cloud, n_views, width, height, first, index_base=0):
    """eg3d_host_dedup_keep: (uint8 mask of the cloud against the map as it stands, n_kept)."""
    ep = D.EdgePointsArrays(cloud)
    if first.dtype != np.uint32 or not first.flags["C_CONTIGUOUS"] or first.size != lib().eg3d_host_dedup_n_cells(n_views, width, height):
        raise ValueError("first must be a contiguous uint32 map of this rig")
    n = int(cloud["n_points"])
    keep, n_kept = np.zeros(max(n, 1), np.uint8), C.c_uint64(0)
    rc = lib().eg3d_host_dedup_keep(n_views, width, height, C.byref(ep.c), int(index_base), D.np_ptr(first, C.c_uint32),
                                    D.np_ptr(keep, C.c_uint8), C.byref(n_kept))
    if rc != 0:
        raise ValueError("eg3d_host_dedup_keep refused the cloud (%d)" % rc)
    return keep[:n], int(n_kept.value)


def dedup_merge(first, other):
    """eg3d_host_dedup_merge: first = min(first, other), in place. Returns first."""
    if first.dtype != np.uint32 or other.dtype != np.uint32 or first.shape != other.shape:
        raise ValueError("two uint32 maps of one shape are needed")
    other = np.ascontiguousarray(other)
    if lib().eg3d_host_dedup_merge(D.np_ptr(first, C.c_uint32), D.np_ptr(other, C.c_uint32), first.size) != 0:
        raise ValueError("eg3d_host_dedup_merge failed")
    return first


def triangulate(cam_P, obs_off, obs_view, obs_xy, X0=None, mode=None, dlt_rows=3, n_threads=1):
    """eg3d_host_triangulate (include/eg3d_host_triangulate.h): the host statement of Context.triangulate, without a GPU.
    cam_P [V, 16]; dlt_rows 3 = the 6x4 DLT system (libeg3d.so), 2 = the 4x4 one (libeg3d_dlt4x4.so); mode 0 = DLT then
    Gauss-Newton, 1 = Gauss-Newton from X0 (the default when X0 is given). Returns (X [n, 3] float32, valid [n] uint8,
    flags [n] uint8: 1 short, 2 degenerate DLT pair). Raises ValueError when the arguments are refused."""
    if mode is None:
        mode = 0 if X0 is None else 1
    P = np.ascontiguousarray(np.asarray(cam_P, np.float32).reshape(-1, 16))
    obs_off = np.ascontiguousarray(obs_off, np.uint32)
    obs_view = np.ascontiguousarray(obs_view, np.int32)
    obs_xy = np.ascontiguousarray(obs_xy, np.float32)
    n = len(obs_off) - 1
    x0 = None if X0 is None else np.ascontiguousarray(X0, np.float32)
    X, valid, flags = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    rc = lib().eg3d_host_triangulate(int(dlt_rows), D.np_ptr(P, C.c_float), len(P), int(mode), n, D.np_ptr(obs_off, C.c_uint32),
                                     D.np_ptr(obs_view, C.c_int32), D.np_ptr(obs_xy, C.c_float),
                                     None if x0 is None else D.np_ptr(x0, C.c_float), int(n_threads), D.np_ptr(X, C.c_float),
                                     D.np_ptr(valid, C.c_uint8), D.np_ptr(flags, C.c_uint8))
    if rc != 0:
        raise ValueError("eg3d_host_triangulate refused its arguments (rc=%d)" % rc)
    return X, valid, flags


def colour_points(images, obs_off, obs_view, obs_xy, keep=None, n_threads=1):
    """eg3d_host_colour_points (include/eg3d_host_colour.h): the host statement of Context.colour_points / colour_device,
    without a GPU. images: one [H, W, 3] uint8 RGB array or None per view. Returns (rgb [n, 3] uint8, flags [n] uint8,
    counts dict: n_coloured, n_empty, n_obs_sampled). Raises ValueError when the arguments are refused."""
    a = D.ImageArgs(images)
    obs_off = np.ascontiguousarray(obs_off, np.uint32)
    obs_view = np.ascontiguousarray(obs_view, np.int32)
    obs_xy = np.ascontiguousarray(obs_xy, np.float32)
    n = len(obs_off) - 1
    k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    rgb, flags, counts = np.zeros((n, 3), np.uint8), np.zeros(n, np.uint8), np.zeros(3, np.uint64)
    rc = lib().eg3d_host_colour_points(*a.args(), n, D.np_ptr(obs_off, C.c_uint32), D.np_ptr(obs_view, C.c_int32),
                                       D.np_ptr(obs_xy, C.c_float), None if k is None else D.np_ptr(k, C.c_uint8), int(n_threads),
                                       D.np_ptr(rgb, C.c_uint8), D.np_ptr(flags, C.c_uint8), D.np_ptr(counts, C.c_uint64))
    if rc != 0:
        raise ValueError("eg3d_host_colour_points refused its arguments (rc=%d)" % rc)
    return rgb, flags, {"n_coloured": int(counts[0]), "n_empty": int(counts[1]), "n_obs_sampled": int(counts[2])}


# ---- include/eg3d_host_transform.h: the similarity fit to known camera centres and its application ----
class TransformError(ValueError):
    """A refusal of include/eg3d_host_transform.h; `rc` is its EG3D_TRANSFORM_ERR_* code."""

    def __init__(self, what, rc):
        ValueError.__init__(self, "%s refused its arguments (rc=%d)" % (what, rc))
        self.rc = rc


TRANSFORM_ERR_ARG, TRANSFORM_ERR_FEW, TRANSFORM_ERR_DEGENERATE = -1, -2, -3
TRANSFORM_ERR_NONFINITE, TRANSFORM_ERR_FILE, TRANSFORM_ERR_SHORT = -4, -5, -6


def _T16(T):
    T = np.ascontiguousarray(T, np.float64).reshape(-1)
    if T.size != 16:
        raise ValueError("T must hold 16 values (a row-major 4 x 4)")
    return T


def read_camera_poses(path, n_cameras):
    """eg3d_host_read_camera_poses: [n_cameras, 3] float64; TransformError (rc -5 unreadable, -6 short) otherwise."""
    out = np.zeros((int(n_cameras), 3), np.float64)
    rc = lib().eg3d_host_read_camera_poses(os.fsencode(path), int(n_cameras), D.np_ptr(out, C.c_double))
    if rc != 0:
        raise TransformError("eg3d_host_read_camera_poses", rc)
    return out


def null_cameras(R, C3):
    """eg3d_host_null_cameras: uint8 [n], 1 where the centre and the whole rotation are exactly 0."""
    R = np.ascontiguousarray(R, np.float32).reshape(-1, 9)
    C3 = np.ascontiguousarray(C3, np.float32).reshape(-1, 3)
    mask = np.zeros(len(R), np.uint8)
    if len(R) != len(C3) or lib().eg3d_host_null_cameras(len(R), D.np_ptr(R, C.c_float), D.np_ptr(C3, C.c_float),
                                                         D.np_ptr(mask, C.c_uint8)) != 0:
        raise ValueError("null_cameras: R and C differ in length")
    return mask


def similarity_fit(src, dst, null_mask=None):
    """eg3d_host_similarity_fit: (T [4, 4] float64, stats dict: n_used, scale, singular [3], src_var, reflection,
    rank_deficient). TransformError with rc -2 (fewer than 3 cameras), -3 (all source centres equal), -4 (a NaN / inf)."""
    src = np.ascontiguousarray(src, np.float64).reshape(-1, 3)
    dst = np.ascontiguousarray(dst, np.float64).reshape(-1, 3)
    m = None if null_mask is None else np.ascontiguousarray(null_mask, np.uint8).reshape(-1)
    if len(src) != len(dst) or (m is not None and len(m) != len(src)):
        raise ValueError("similarity_fit: src, dst and null_mask differ in length")
    T = np.zeros(16, np.float64)
    st = D.SimilarityStats(struct_size=C.sizeof(D.SimilarityStats))
    rc = lib().eg3d_host_similarity_fit(len(src), D.np_ptr(src, C.c_double), D.np_ptr(dst, C.c_double),
                                        None if m is None else D.np_ptr(m, C.c_uint8), D.np_ptr(T, C.c_double), C.byref(st))
    if rc != 0:
        raise TransformError("eg3d_host_similarity_fit", rc)
    return T.reshape(4, 4), {"n_used": st.n_used, "scale": st.scale, "singular": np.array(st.singular[:]), "src_var": st.src_var,
                             "reflection": bool(st.reflection), "rank_deficient": bool(st.rank_deficient)}


def transform_points(T, X, out=None):
    """eg3d_host_transform_points: X [n, 3] float32 through T (row-major 4 x 4, float64) — the sequential statement of
    Context.transform_device / transform_points. out may be X itself (in place)."""
    T = _T16(T)
    X = np.ascontiguousarray(X, np.float32).reshape(-1, 3)
    if out is None:
        out = np.empty_like(X)
    if out.dtype != np.float32 or out.shape != X.shape or not out.flags.c_contiguous:
        raise ValueError("transform_points: out must be a contiguous float32 array shaped like X")
    rc = lib().eg3d_host_transform_points(D.np_ptr(T, C.c_double), D.np_ptr(X, C.c_float), len(X), D.np_ptr(out, C.c_float))
    if rc != 0:
        raise TransformError("eg3d_host_transform_points", rc)
    return out


def transform_cameras(T, fpp, R, C3, t):
    """eg3d_host_transform_cameras on copies: fpp [n, 3] (focal, ppx, ppy), R [n, 9], C [n, 3], t [n, 3] ->
    (R', C', t', P [n, 16]); the rows of a null camera come back unchanged and its P as zeros."""
    T = _T16(T)
    fpp = np.ascontiguousarray(fpp, np.float32).reshape(-1, 3)
    R = np.array(R, np.float32).reshape(-1, 9)
    C3 = np.array(C3, np.float32).reshape(-1, 3)
    t = np.array(t, np.float32).reshape(-1, 3)
    n = len(fpp)
    if not (len(R) == len(C3) == len(t) == n):
        raise ValueError("transform_cameras: the arrays differ in length")
    P = np.zeros((n, 16), np.float32)
    rc = lib().eg3d_host_transform_cameras(D.np_ptr(T, C.c_double), n, D.np_ptr(fpp, C.c_float), D.np_ptr(R, C.c_float),
                                           D.np_ptr(C3, C.c_float), D.np_ptr(t, C.c_float), D.np_ptr(P, C.c_float))
    if rc != 0:
        raise TransformError("eg3d_host_transform_cameras", rc)
    return R, C3, t, P


def glm_inverse4(m):
    m = np.ascontiguousarray(m, np.float32).reshape(16)
    out = np.zeros(16, np.float32)
    lib().eg3d_host_glm_inverse4(D.np_ptr(m, C.c_float), D.np_ptr(out, C.c_float))
    return out.reshape(4, 4)


def glm_mul4(a, b):
    a, b = np.ascontiguousarray(a, np.float32).reshape(16), np.ascontiguousarray(b, np.float32).reshape(16)
    out = np.zeros(16, np.float32)
    lib().eg3d_host_glm_mul4(D.np_ptr(a, C.c_float), D.np_ptr(b, C.c_float), D.np_ptr(out, C.c_float))
    return out.reshape(4, 4)


def camera_errors(C3, target, null_mask=None):
    """eg3d_host_camera_errors: the reference's mean camera position error as a float — the sum runs over the non-null
    cameras, the division is by ALL cameras."""
    C3 = np.ascontiguousarray(C3, np.float32).reshape(-1, 3)
    target = np.ascontiguousarray(target, np.float64).reshape(-1, 3)
    m = None if null_mask is None else np.ascontiguousarray(null_mask, np.uint8).reshape(-1)
    if len(C3) != len(target) or (m is not None and len(m) != len(C3)):
        raise ValueError("camera_errors: the arrays differ in length")
    out = C.c_float(0)
    rc = lib().eg3d_host_camera_errors(len(C3), D.np_ptr(C3, C.c_float), None if m is None else D.np_ptr(m, C.c_uint8),
                                       D.np_ptr(target, C.c_double), C.byref(out))
    if rc != 0:
        raise TransformError("eg3d_host_camera_errors", rc)
    return np.float32(out.value)


def write_ply(path, X, rgb=None, keep=None):
    """eg3d_host_write_ply: the reference's ASCII PLY point cloud of X [n, 3]; rgb [n, 3] uint8 or None (white); keep [n]
    or None (all) — the `inliers` forms."""
    X = np.ascontiguousarray(X, np.float32).reshape(-1, 3)
    n = len(X)
    c = None if rgb is None else np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    k = None if keep is None else np.ascontiguousarray(keep, np.uint8).reshape(-1)
    if (c is not None and len(c) != n) or (k is not None and len(k) != n):
        raise ValueError("write_ply: X, rgb and keep differ in length")
    rc = lib().eg3d_host_write_ply(os.fsencode(path), n, D.np_ptr(X, C.c_float) if n else None,
                                   D.np_ptr(c, C.c_uint8) if c is not None and n else None,
                                   D.np_ptr(k, C.c_uint8) if k is not None and n else None)
    if rc != 0:
        raise OSError("eg3d_host_write_ply failed (rc=%d): %s" % (rc, path))


def edge_chains(graph, max_dist, simplify=True):
    """eg3d_host_edge_chains (include/eg3d/host_edges.h): the sequential statement of the 3-D edge model. `graph`: a dict as
    replay_matches returns it (only its geometric half is read). Returns a dict of numpy arrays: chain_off, chain_node,
    flags, s_off, s_node, length, stats. Raises ValueError when the graph or max_dist is refused; .code holds the C code."""
    ga = D.EdgesGraphArrays(graph)
    ch, st = D.EdgeChains(), D.EdgesStats()
    st.struct_size = C.sizeof(D.EdgesStats)
    rc = lib().eg3d_host_edge_chains(C.byref(ga.c), float(max_dist), 1 if simplify else 0, C.byref(ch), C.byref(st))
    if rc != 0:
        err = ValueError("eg3d_host_edge_chains refused its input (%d)" % rc)
        err.code = rc
        raise err
    d = D.edge_chains_to_dict(ch, st)
    lib().eg3d_host_free_edge_chains(C.byref(ch))
    return d


def write_ply_edges(path, chains, node_X):
    """eg3d_host_write_ply_edges: the kept vertices of `chains` (a dict as edge_chains returns it) as an ASCII PLY line model
    with `element vertex` and `element edge`. node_X [n_nodes, 3]: the positions the chains' node ids index."""
    ca = D.EdgeChainsArrays(chains)
    X = np.ascontiguousarray(node_X, np.float32).reshape(-1, 3)
    if len(ca.a["s_node"]) and int(ca.a["s_node"].max()) >= len(X):
        raise ValueError("write_ply_edges: a node id lies outside node_X")
    rc = lib().eg3d_host_write_ply_edges(os.fsencode(path), C.byref(ca.c), D.np_ptr(X, C.c_float) if len(X) else None)
    if rc != 0:
        raise OSError("eg3d_host_write_ply_edges failed (rc=%d): %s" % (rc, path))


# ---- include/eg3d/host_nearest.hpp: cloud-to-cloud nearest distances (K18's sequential statement), the PLY point reader ----
class NearestError(ValueError):
    """A refusal of include/eg3d/host_nearest.hpp; `code` is its EG3D_NEAREST_ERR_* code, the text the library's."""

    def __init__(self, what, code):
        ValueError.__init__(self, "%s refused (rc=%d): %s" % (what, code, lib().eg3d_host_nearest_last_error().decode()))
        self.code = code


NEAREST_ERR_ARG, NEAREST_ERR_CAPACITY, NEAREST_ERR_CELL, NEAREST_ERR_MAXDIST = -1, -3, -18, -19
NEAREST_ERR_THRESHOLD, NEAREST_ERR_EXTENT, NEAREST_ERR_FOREIGN, NEAREST_ERR_FILE, NEAREST_ERR_PLY = -20, -21, -22, -23, -24
NEAREST_NONE = 0xFFFFFFFF


def _points_and_keep(what, X, keep):
    X = np.ascontiguousarray(X, np.float32).reshape(-1, 3)
    k = None if keep is None else np.ascontiguousarray(keep, np.uint8).reshape(-1)
    if k is not None and len(k) != len(X):
        raise ValueError("%s: the points and their keep mask differ in length" % what)
    return X, k


def _opt_ptr(a, ctype):
    return D.np_ptr(a, ctype) if a is not None and len(a) else None


def cloud_nearest(ref_X, X, max_dist, cell=None, ref_keep=None, keep=None, thresholds=(), d2=None, nn=None):
    """eg3d_host_cloud_nearest: for every query X[i] the squared distance (float32; +inf = none) to the nearest reference
    point within max_dist and that point's index (uint32; 0xFFFFFFFF = none). cell: the grid's edge, None = max_dist.
    d2 / nn: arrays to fill (contiguous, [n] float32 / uint32), allocated when not given. Returns (d2, nn, stats dict as
    _cdefs.nearest_stats_to_dict gives it). NearestError when the library refuses."""
    R, rk = _points_and_keep("cloud_nearest", ref_X, ref_keep)
    Q, qk = _points_and_keep("cloud_nearest", X, keep)
    d2 = np.empty(len(Q), np.float32) if d2 is None else d2
    nn = np.empty(len(Q), np.uint32) if nn is None else nn
    if d2.dtype != np.float32 or nn.dtype != np.uint32 or d2.shape != (len(Q),) or nn.shape != (len(Q),):
        raise ValueError("cloud_nearest: d2 / nn must be [n] float32 / uint32")
    st = D.nearest_stats_new(thresholds)
    rc = lib().eg3d_host_cloud_nearest(_opt_ptr(R, C.c_float), len(R), _opt_ptr(rk, C.c_uint8), _opt_ptr(Q, C.c_float), len(Q),
                                       _opt_ptr(qk, C.c_uint8), float(max_dist if cell is None else cell), float(max_dist),
                                       _opt_ptr(d2, C.c_float), _opt_ptr(nn, C.c_uint32), C.byref(st))
    if rc != 0:
        raise NearestError("eg3d_host_cloud_nearest", rc)
    return d2, nn, D.nearest_stats_to_dict(st, max_dist)


def cloud_index_stats(ref_X, cell, ref_keep=None):
    """eg3d_host_cloud_index_stats: what the statement's grid over ref_X looks like (n_indexed, n_cells, origin, dims,
    max_cell_points, ...) — the figures Context.cloud_index reports."""
    R, rk = _points_and_keep("cloud_index_stats", ref_X, ref_keep)
    st = D.CloudIndexStats(struct_size=C.sizeof(D.CloudIndexStats))
    rc = lib().eg3d_host_cloud_index_stats(_opt_ptr(R, C.c_float), len(R), _opt_ptr(rk, C.c_uint8), float(cell), C.byref(st))
    if rc != 0:
        raise NearestError("eg3d_host_cloud_index_stats", rc)
    return D.cloud_index_stats_to_dict(st)


def compare_clouds(X, ref_X, max_dist, thresholds=(), keep=None, ref_keep=None):
    """Both directions of a comparison on the host: {"accuracy": figures of X against ref_X, "completeness": figures of
    ref_X against X}, each a stats dict with `mean` and `median` as distances. The cell is max_dist."""
    return {"accuracy": cloud_nearest(ref_X, X, max_dist, ref_keep=ref_keep, keep=keep, thresholds=thresholds)[2],
            "completeness": cloud_nearest(X, ref_X, max_dist, ref_keep=keep, keep=ref_keep, thresholds=thresholds)[2]}


def read_ply_points(path):
    """eg3d_host_read_ply_points: the `element vertex` of an ASCII or binary little-endian PLY file as [n, 3] float32.
    NearestError (code -23: the file cannot be read; -24: the file is refused, the text says why)."""
    X, n = D.f32p(), C.c_uint64(0)
    rc = lib().eg3d_host_read_ply_points(os.fsencode(path), C.byref(X), C.byref(n))
    if rc != 0:
        raise NearestError("eg3d_host_read_ply_points", rc)
    out = D.as_np(X, 3 * n.value, np.float32).reshape(-1, 3)
    lib().eg3d_host_free_points(X)
    return out


def read_png_rgb(path):
    """eg3d_host_png_read_rgb: a non-interlaced PNG of any colour type and bit depth as an [H, W, 3] uint8 RGB array."""
    w, h, p = C.c_int(0), C.c_int(0), D.u8p()
    rc = lib().eg3d_host_png_read_rgb(os.fsencode(path), C.byref(w), C.byref(h), C.byref(p))
    if rc != 0:
        raise ValueError("eg3d_host_png_read_rgb failed (rc=%d): %s" % (rc, path))
    try:
        return D.as_np(p, w.value * h.value * 3, np.uint8).reshape(h.value, w.value, 3)
    finally:
        lib().eg3d_host_free(p)


def is_matched(scene_ptr, graph, view, pl, seg, xy):
    """PLGMatchesManager::is_matched for n points against the matched intervals of `graph` (a dict as returned by
    replay_matches): int64 [n], -1 or the index within its row of the interval that contains the point
    (eg3d_host_is_matched — the rule the kernels of Context.match_polyline_sets(matched=...) apply). Raises ValueError
    when the intervals fail their checks or the extractor's walk would not advance past one of them."""
    m = D.MatchedIntervalsArrays(graph)
    view = np.ascontiguousarray(view, np.int32).reshape(-1)
    n = len(view)
    pad = lambda a, t, w: np.ascontiguousarray(a, t).reshape(-1) if n else np.zeros(w, t)
    pl, seg, xy = pad(pl, np.uint32, 1), pad(seg, np.uint32, 1), pad(xy, np.float32, 2)
    if n and (len(pl) != n or len(seg) != n or len(xy) != 2 * n):
        raise ValueError("is_matched: view, pl, seg, xy differ in length")
    out = np.full(max(n, 1), -1, np.int64)
    rc = lib().eg3d_host_is_matched(scene_ptr, C.byref(m.c), n, D.np_ptr(view if n else np.zeros(1, np.int32), C.c_int32),
                                    D.np_ptr(pl, C.c_uint32), D.np_ptr(seg, C.c_uint32), D.np_ptr(xy, C.c_float),
                                    D.np_ptr(out, C.c_int64))
    if rc == -2:
        raise ValueError("is_matched: the intervals do not belong to this scene (the walk would not advance past %d of the "
                         "points)" % int((out[:n] <= -2).sum()))
    if rc != 0:
        raise ValueError("is_matched: bad intervals or points (%d)" % rc)
    return out[:n]


def write_compat_graph(path, graph):
    """Pipeline 1's compatibility graph (a dict as returned by Context.similarity_graph) as the text file the reference
    hands to its community detection (eg3d_host_write_compat_graph)."""
    g = D.SimgraphArrays(graph)
    rc = lib().eg3d_host_write_compat_graph(os.fsencode(path), C.byref(g.c))
    if rc != 0:
        raise RuntimeError("eg3d_host_write_compat_graph(%s) failed (%d)" % (path, rc))


def read_communities(path):
    """One community id per node, as the reference reads its community detection's output (int64 array)."""
    ids, n = C.POINTER(C.c_int64)(), C.c_uint64()
    rc = lib().eg3d_host_read_communities(os.fsencode(path), C.byref(ids), C.byref(n))
    if rc != 0:
        raise RuntimeError("eg3d_host_read_communities(%s) failed (%d)" % (path, rc))
    out = D.as_np(ids, n.value, np.int64)
    lib().eg3d_host_free(ids)
    return out


def write_communities(path, ids):
    """One community id per line, as Grappolo writes the file the reference reads (eg3d_host_write_communities)."""
    ids = np.ascontiguousarray(ids, np.int64)
    buf = ids if len(ids) else np.zeros(1, np.int64)
    rc = lib().eg3d_host_write_communities(os.fsencode(path), D.np_ptr(buf, C.c_int64), len(ids))
    if rc != 0:
        raise RuntimeError("eg3d_host_write_communities(%s) failed (%d)" % (path, rc))


def sets_from_communities(graph, ids, n_views):
    """The polyline sets of pipeline 1 from the graph's nodes and one community id per node: (n_sets, row_off, pl_ids), the
    CSR Context.match_polyline_sets takes. A negative id leaves its node out; a wrong number of ids is refused."""
    g = D.SimgraphArrays(graph)
    ids = np.ascontiguousarray(ids, np.int64)
    buf = ids if len(ids) else np.zeros(1, np.int64)
    ps = D.PolylineSets()
    rc = lib().eg3d_host_sets_from_communities(C.byref(g.c), D.np_ptr(buf, C.c_int64), len(ids), n_views, C.byref(ps))
    if rc != 0:
        raise RuntimeError("eg3d_host_sets_from_communities failed (%d)" % rc)
    n_sets = int(ps.n_sets)
    row_off = D.as_np(ps.row_off, n_sets * n_views + 1, np.uint32)
    pl_ids = D.as_np(ps.pl_ids, int(row_off[-1]), np.uint32)
    lib().eg3d_host_free_polyline_sets(C.byref(ps))
    return n_sets, row_off, pl_ids


def plg_from_mask(mask):
    """binary edge image (uint8 [h, w], non-zero = edge) -> optimised polyline graph of one view."""
    m = np.ascontiguousarray(mask, np.uint8)
    v = D.PlgView()
    rc = lib().eg3d_plg_build_from_mask(D.np_ptr(m, C.c_uint8), m.shape[1], m.shape[0], C.byref(v))
    if rc != 0:
        raise RuntimeError("eg3d_plg_build_from_mask failed (%d)" % rc)
    d = D.plg_view_to_dict(v)
    lib().eg3d_plg_view_free(C.byref(v))
    return d


def estimate_F(n_views, trk_off, trk_view, trk_xy, estimate=True, rng_seed=0):
    """SURVEY N4 (geometric_utilities.cpp:754-820): fundamental matrices of all ordered view pairs from the
    point tracks; pairs with fewer than 10 common points are invalid. Returns (F [V,V,9] f64, valid [V,V] u8,
    n_common [V,V] u32, pairs whose estimate failed). estimate=False: validity rule and counts only."""
    off = np.ascontiguousarray(trk_off, np.uint32)
    view = np.ascontiguousarray(trk_view, np.int32)
    xy = np.ascontiguousarray(trk_xy, np.float32)
    V = int(n_views)
    F = np.zeros((V, V, 9), np.float64)
    valid = np.zeros((V, V), np.uint8)
    ncom = np.zeros((V, V), np.uint32)
    rc = lib().eg3d_host_estimate_F(V, len(off) - 1, D.np_ptr(off, C.c_uint32), D.np_ptr(view, C.c_int32),
                                    D.np_ptr(xy, C.c_float), 1 if estimate else 0, rng_seed, D.np_ptr(F, C.c_double),
                                    D.np_ptr(valid, C.c_uint8), D.np_ptr(ncom, C.c_uint32))
    if rc < 0:
        raise RuntimeError("eg3d_host_estimate_F failed (%d)" % rc)
    return F, valid, ncom, rc


def estimate_fundamental(n_views, seeds, iterations=0, rng_seed=0, fit_budget=0, stage_points=0):
    """The host statement of api.estimate_fundamental (eg3d_host_estimate_fundamental): the same arguments (fit_budget and
    stage_points have no meaning here), the same return shape, the same bits — without a GPU."""
    rc, out = D.fund_call(lib().eg3d_host_estimate_fundamental, n_views, seeds, iterations, rng_seed, fit_budget, stage_points)
    if rc != 0:
        raise RuntimeError("eg3d_host_estimate_fundamental failed (%d)" % rc)
    return out


def png_edge_mask(path):
    w, h, p = C.c_int(), C.c_int(), D.u8p()
    rc = lib().eg3d_png_read_edge_mask(path.encode(), C.byref(w), C.byref(h), C.byref(p))
    if rc != 0:
        raise RuntimeError("eg3d_png_read_edge_mask(%s) failed (%d)" % (path, rc))
    m = D.as_np(p, w.value * h.value, np.uint8).reshape(h.value, w.value)
    lib().eg3d_host_free(p)
    return m


def edge_maps(images, low, high, smooth_passes=1, l2=False, device=0):
    """The host statement of api.edge_maps (eg3d_host_edge_maps): the same arguments (`device` has no meaning here), the
    same return shape, the same bits — without a GPU."""
    rc, out = D.edgemap_call(lib().eg3d_host_edge_maps, images, low, high, smooth_passes, l2)
    if rc != 0:
        raise RuntimeError("eg3d_host_edge_maps failed (%d): %s" % (rc, lib().eg3d_host_edgemap_last_error().decode()))
    return out


def write_png_mask(path, mask):
    """A mask (uint8 [H, W], non-zero = edge) as a 1-bit greyscale PNG, white = edge (eg3d_host_png_write_mask): what
    png_edge_mask and the N2 builder read."""
    m = np.ascontiguousarray(mask, np.uint8)
    if m.ndim != 2:
        raise ValueError("a mask must be [H, W], not %r" % (m.shape,))
    rc = lib().eg3d_host_png_write_mask(os.fsencode(path), D.np_ptr(m, C.c_uint8), m.shape[1], m.shape[0])
    if rc != 0:
        raise RuntimeError("eg3d_host_png_write_mask(%s) failed (%d): %s" % (path, rc, lib().eg3d_host_edgemap_last_error().decode()))


def plg_views_from_masks(masks):
    """The polyline graphs of many masks at once (eg3d_host_plg_build_views_from_masks), built concurrently on the host's
    cores: a list with what plg_from_mask returns for each mask."""
    ms = [np.ascontiguousarray(m, np.uint8) for m in masks]
    for m in ms:
        if m.ndim != 2:
            raise ValueError("a mask must be [H, W], not %r" % (m.shape,))
    n = len(ms)
    w = np.array([m.shape[1] for m in ms], np.int32)
    h = np.array([m.shape[0] for m in ms], np.int32)
    ptrs = (D.u8p * max(n, 1))(*[D.np_ptr(m, C.c_uint8) for m in ms])
    views = (D.PlgView * max(n, 1))()
    rc = lib().eg3d_host_plg_build_views_from_masks(ptrs, n, D.np_ptr(w, C.c_int32), D.np_ptr(h, C.c_int32), views)
    if rc != 0:
        raise RuntimeError("eg3d_host_plg_build_views_from_masks failed (%d): %s" % (rc, lib().eg3d_host_edgemap_last_error().decode()))
    out = [D.plg_view_to_dict(views[v]) for v in range(n)]
    for v in range(n):
        lib().eg3d_plg_view_free(C.byref(views[v]))
    return out


def build_grid(scene_ptr, view, cell_dim):
    ncols, nrows, dropped = C.c_uint32(), C.c_uint32(), C.c_uint32()
    off, ids = D.u32p(), D.u32p()
    rc = lib().eg3d_host_build_grid(scene_ptr, view, cell_dim, C.byref(ncols), C.byref(nrows), C.byref(off),
                                    C.byref(ids), C.byref(dropped))
    if rc != 0:
        raise RuntimeError("eg3d_host_build_grid failed")
    n = ncols.value * nrows.value
    o = D.as_np(off, n + 1, np.uint32)
    i = D.as_np(ids, int(o[-1]), np.uint32)
    lib().eg3d_host_free(off)
    lib().eg3d_host_free(ids)
    return ncols.value, nrows.value, o, i, dropped.value


class SeedsArrays:
    """Owns numpy copies of a seed set and exposes a ctypes Seeds struct over them."""

    def __init__(self, trk_off, trk_view, trk_xy):
        self.trk_off = np.ascontiguousarray(trk_off, dtype=np.uint32)
        self.trk_view = np.ascontiguousarray(trk_view, dtype=np.int32)
        self.trk_xy = np.ascontiguousarray(trk_xy, dtype=np.float32).reshape(-1, 2)
        self.c = D.Seeds(len(self.trk_off) - 1, D.np_ptr(self.trk_off, C.c_uint32), D.np_ptr(self.trk_view, C.c_int32),
                         D.np_ptr(self.trk_xy, C.c_float))


class SceneArrays:
    """Owns numpy arrays of a scene and exposes a ctypes Scene struct over them."""

    def __init__(self, d):
        self.d = {
            "cam_P": np.ascontiguousarray(d["cam_P"], np.float32), "F": np.ascontiguousarray(d["F"], np.float64),
            "F_valid": np.ascontiguousarray(d["F_valid"], np.uint8),
            "view_pl_off": np.ascontiguousarray(d["view_pl_off"], np.uint32),
            "pl_vtx_off": np.ascontiguousarray(d["pl_vtx_off"], np.uint32),
            "vtx_xy": np.ascontiguousarray(d["vtx_xy"], np.float32),
            "pl_start": np.ascontiguousarray(d["pl_start"], np.uint32),
            "pl_end": np.ascontiguousarray(d["pl_end"], np.uint32),
            "pl_valid": np.ascontiguousarray(d["pl_valid"], np.uint8),
        }
        a = self.d
        self.c = D.Scene(int(d["n_views"]), int(d["width"]), int(d["height"]), D.np_ptr(a["cam_P"], C.c_float),
                         D.np_ptr(a["F"], C.c_double), D.np_ptr(a["F_valid"], C.c_uint8),
                         D.np_ptr(a["view_pl_off"], C.c_uint32), D.np_ptr(a["pl_vtx_off"], C.c_uint32),
                         D.np_ptr(a["vtx_xy"], C.c_float), D.np_ptr(a["pl_start"], C.c_uint32),
                         D.np_ptr(a["pl_end"], C.c_uint32), D.np_ptr(a["pl_valid"], C.c_uint8))
