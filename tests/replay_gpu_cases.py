"""What the GPU tests of the device replay (eg3d_replay_device) share: a three-view scene of a few polylines, one small
hand-built cloud per rule of host/replay.cpp, the upload of a cloud as caller-built device arrays, the comparison of two
graphs, and - run as a script - the child process of the table-stress test (EG3D_REPLAY_TABLE_BITS is read when a context
is created)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from edgegraph3d_amd import _cdefs as D  # noqa: E402
from edgegraph3d_amd import api, host  # noqa: E402

FIELDS = ("n_nodes", "n_real_nodes", "n_polylines")
ARRAYS = ("node_X", "node_point", "pl_start", "pl_end", "conn_off", "conn_pl", "iv_off", "iv_start_seg", "iv_start_xy",
          "iv_end_seg", "iv_end_xy")


def same_graph(a, b):
    """None if the two graphs are equal field for field and bit for bit, else the name of the first field that differs."""
    for f in FIELDS:
        if a[f] != b[f]:
            return f
    for f in ARRAYS:
        x, y = a[f], b[f]
        if x.dtype != y.dtype or x.shape != y.shape:
            return f + " (shape / dtype)"
        if not np.array_equal(x.view(np.uint32) if x.dtype.kind == "f" else x, y.view(np.uint32) if y.dtype.kind == "f" else y):
            return f
    return None


# ---- the scene: cameras of synthetic config 0 (three views), polylines of its own --------------------------------------
# view 0:  P0 (10,10) (20,10) (30,10) (40,10) (50,10)   nodes 0 -> 1
#          P1 (50,10) (60,20) (70,30)                   nodes 1 -> 2   (starts on P0's end node)
#          P2 (5,60) (5,40) (10,10)                     nodes 3 -> 0   (ends on P0's start node)
#          P3 (80,80) (90,80)                           nodes 4 -> 5   (shares nothing)
# view 1:  Q0 (10,50) (20,50) (30,50) (40,50)           nodes 0 -> 1
#          Q1 (100,100) (110,100)                       nodes 2 -> 3
# view 2:  R0 (10,90) (30,90) (50,90)                   nodes 0 -> 1
POLYLINES = [
    [([(10, 10), (20, 10), (30, 10), (40, 10), (50, 10)], 0, 1), ([(50, 10), (60, 20), (70, 30)], 1, 2),
     ([(5, 60), (5, 40), (10, 10)], 3, 0), ([(80, 80), (90, 80)], 4, 5)],
    [([(10, 50), (20, 50), (30, 50), (40, 50)], 0, 1), ([(100, 100), (110, 100)], 2, 3)],
    [([(10, 90), (30, 90), (50, 90)], 0, 1)],
]
P0, P1, P2, P3 = 0, 1, 2, 3
Q0, Q1 = 0, 1
R0 = 0


def small_scene():
    """host.SceneArrays of the scene above (keep the object: it owns the arrays the ctypes struct points into)."""
    base = host.Synth(0).scene_np()
    V = len(POLYLINES)
    assert base["n_views"] >= V
    vpo, pvo, vtx, ps, pe = [0], [0], [], [], []
    for view in POLYLINES:
        for verts, a, b in view:
            vtx.extend(verts)
            pvo.append(len(vtx))
            ps.append(a)
            pe.append(b)
        vpo.append(len(ps))
    return host.SceneArrays({
        "n_views": V, "width": base["width"], "height": base["height"], "cam_P": base["cam_P"][:V].copy(),
        "F": base["F"][:V, :V].copy(), "F_valid": base["F_valid"][:V, :V].copy(), "view_pl_off": np.array(vpo, np.uint32),
        "pl_vtx_off": np.array(pvo, np.uint32), "vtx_xy": np.array(vtx, np.float32), "pl_start": np.array(ps, np.uint32),
        "pl_end": np.array(pe, np.uint32), "pl_valid": np.ones(len(ps), np.uint8)})


def global_pl(view, pl):
    return sum(len(v) for v in POLYLINES[:view]) + pl


def make_cloud(points):
    """points = list of (X, [(view, pl, seg, x, y) ...], key4) -> a cloud dict (obs_off with its sentinel)."""
    n = len(points)
    X = np.array([p[0] for p in points], np.float32).reshape(n, 3)
    off, view, pl, seg, xy, key = [0], [], [], [], [], []
    for _, obs, k in points:
        for (v, p, s, x, y) in obs:
            view.append(v), pl.append(p), seg.append(s), xy.append((x, y))
        off.append(len(view))
        key.append(k)
    return {"n_points": n, "n_obs": len(view), "X": X, "obs_off": np.array(off, np.uint64),
            "obs_view": np.array(view, np.int32), "obs_pl": np.array(pl, np.uint32), "obs_seg": np.array(seg, np.uint32),
            "obs_xy": np.array(xy, np.float32).reshape(-1, 2), "key": np.array(key, np.uint32).reshape(-1, 4)}


A, B, Cc, Dd = (1.0, 2.0, 3.0), (4.0, 5.0, 6.0), (7.0, 8.0, 9.0), (1.5, 2.5, 3.5)
ZP, ZN = (0.0, 1.0, 1.0), (-0.0, 1.0, 1.0)


def cases():
    """name -> cloud. Observations lie ON their segments (the replay reads, never projects)."""
    c = {}
    # (a) one X in two chains: nodes A0 B1 C2, A's node_point is its last lookup (point 3)
    c["a_shared_node"] = make_cloud([
        (A, [(0, P0, 0, 12, 10)], (0, 0, 0, 0)), (B, [(0, P0, 1, 22, 10)], (0, 0, 0, 1)),
        (Cc, [(1, Q0, 0, 12, 50)], (1, 0, 0, 0)), (A, [(1, Q0, 1, 22, 50)], (1, 0, 0, 1))])
    # (b) the same connection in both orientations, in different chains: one polyline, oriented A -> B
    c["b_both_orientations"] = make_cloud([
        (A, [(0, P0, 0, 12, 10)], (0, 0, 0, 0)), (B, [(0, P0, 1, 22, 10)], (0, 0, 0, 1)),
        (B, [(1, Q0, 0, 12, 50)], (1, 0, 0, 0)), (A, [(1, Q0, 1, 22, 50)], (1, 0, 0, 1)),
        (B, [], (2, 0, 0, 0)), (Cc, [], (2, 0, 0, 1)), (B, [], (2, 0, 0, 2))])
    # (c) consecutive points with identical X: the loop (A, A), linked once, then A -> B
    c["c_loop"] = make_cloud([
        (A, [(0, P0, 0, 12, 10)], (0, 0, 0, 0)), (A, [(0, P0, 1, 22, 10)], (0, 0, 0, 1)),
        (B, [(0, P0, 2, 32, 10)], (0, 0, 0, 2)), (A, [], (0, 0, 0, 3)), (A, [], (0, 0, 0, 4))])
    # (d) -0.0 and +0.0 are one node; node_X keeps the bits of the first lookup (-0.0 here)
    c["d_signed_zero"] = make_cloud([
        (ZN, [(0, P0, 0, 12, 10)], (0, 0, 0, 0)), (B, [(0, P0, 1, 22, 10)], (0, 0, 0, 1)),
        (ZP, [(0, P0, 2, 32, 10)], (0, 0, 0, 2)), (ZN, [], (1, 0, 0, 0)), (ZP, [], (1, 0, 0, 1))])
    # (e) intervals with one (polyline, start segment): the earlier pair wins, whatever the later pairs bring; a pair that
    #     sees two views inserts one interval per view (keys of different views never meet: the polyline is per view)
    c["e_first_interval_wins"] = make_cloud([
        (A, [(0, P0, 0, 12, 10), (1, Q0, 0, 12, 50)], (0, 0, 0, 0)),
        (B, [(0, P0, 2, 32, 10), (1, Q0, 2, 32, 50)], (0, 0, 0, 1)),          # P0: 0 -> 2, Q0: 0 -> 2
        (Cc, [(0, P0, 0, 18, 10), (1, Q0, 1, 22, 50)], (1, 0, 0, 0)),
        (Dd, [(0, P0, 1, 22, 10), (1, Q0, 0, 14, 50)], (1, 0, 0, 1)),         # P0: 0 -> 1 loses; Q0: (swapped) 0 -> 1 loses
        (Dd, [(0, P0, 3, 42, 10)], (2, 0, 0, 0)), (A, [(0, P0, 0, 11, 10)], (2, 0, 0, 1))])   # P0: swapped 0 -> 3 loses
    # (f) both observations on one segment: ordered from the segment's first vertex, in both directions, and coincident
    c["f_same_segment"] = make_cloud([
        (A, [(0, P0, 1, 22, 10)], (0, 0, 0, 0)), (B, [(0, P0, 1, 28, 10)], (0, 0, 0, 1)),     # as given
        (Cc, [(0, P0, 2, 38, 10)], (1, 0, 0, 0)), (Dd, [(0, P0, 2, 32, 10)], (1, 0, 0, 1)),   # swapped
        (A, [(2, R0, 0, 20, 90)], (2, 0, 0, 0)), (Cc, [(2, R0, 0, 20, 90)], (2, 0, 0, 1)),    # the same point: ordered
        (B, [(0, P1, 1, 68, 28)], (3, 0, 0, 0)), (Dd, [(0, P1, 1, 62, 22)], (3, 0, 0, 1))])   # swapped, decided by y too
    # (g) observations on different polylines that share an extreme node
    c["g_shared_extreme"] = make_cloud([
        # start extreme: the first point sits on P0's start (node 0), which is P2's END: interval on P2 from its last vertex
        (A, [(0, P0, 0, 10, 10)], (0, 0, 0, 0)), (B, [(0, P2, 0, 5, 50)], (0, 0, 0, 1)),
        # end extreme: the first point sits on P0's end (node 1), which is P1's START: interval on P1 from its first vertex
        (Cc, [(0, P0, 3, 50, 10)], (1, 0, 0, 0)), (Dd, [(0, P1, 1, 65, 25)], (1, 0, 0, 1)),
        # not on an extreme: nothing; on an extreme the other polyline does not share: nothing
        (A, [(0, P0, 0, 15, 10)], (2, 0, 0, 0)), (Dd, [(0, P2, 1, 6, 34)], (2, 0, 0, 1)),
        (B, [(0, P0, 3, 50, 10)], (3, 0, 0, 0)), (Cc, [(0, P3, 0, 85, 80)], (3, 0, 0, 1)),
        # on segment 0 but not AT the start vertex / at the end vertex's coordinates but on another segment: nothing
        (B, [(0, P0, 0, 10, 10.5)], (4, 0, 0, 0)), (A, [(0, P2, 1, 7, 28)], (4, 0, 0, 1))])
    # (h) one point lists a view twice: the last observation of that view counts, in the first and in the second point
    c["h_repeated_view"] = make_cloud([
        (A, [(0, P0, 3, 42, 10), (1, Q0, 0, 12, 50), (0, P0, 0, 12, 10)], (0, 0, 0, 0)),
        (B, [(0, P0, 1, 22, 10), (1, Q0, 2, 32, 50), (1, Q0, 1, 22, 50), (0, P0, 2, 32, 10)], (0, 0, 0, 1))])
    # (i) degenerate inputs
    c["i_empty"] = make_cloud([])
    c["i_one_point_chains"] = make_cloud([
        (A, [(0, P0, 0, 12, 10)], (0, 0, 0, 0)), (B, [(0, P0, 1, 22, 10)], (1, 0, 0, 0)), (A, [], (1, 1, 0, 0)),
        (Cc, [(1, Q0, 0, 12, 50)], (1, 1, 1, 0))])
    # (j) a key[3] that does not count up starts a new chain: A | B -> C only
    c["j_key_gap"] = make_cloud([
        (A, [(0, P0, 0, 12, 10)], (0, 0, 0, 0)), (B, [(0, P0, 1, 22, 10)], (0, 0, 0, 2)),
        (Cc, [(0, P0, 2, 32, 10)], (0, 0, 0, 3)), (Dd, [(0, P0, 3, 42, 10)], (0, 0, 0, 3))])
    return c


def upload_cloud(ctx, cloud):
    """The cloud as caller-built device arrays: (DeviceEdgePoints, the DeviceArrays that own the memory)."""
    arrays = {"X": cloud["X"], "obs_off": cloud["obs_off"][:-1], "obs_view": cloud["obs_view"], "obs_pl": cloud["obs_pl"],
              "obs_seg": cloud["obs_seg"], "obs_xy": cloud["obs_xy"], "key": cloud["key"]}
    held = {k: ctx.upload(v) for k, v in arrays.items()}
    d = D.DeviceEdgePoints()
    d.n_points, d.n_obs, d.complete = int(cloud["n_points"]), int(cloud["n_obs"]), 1
    for k, a in held.items():
        setattr(d, k, a.ptr)
    return d, held


def config0_graph():
    """The replay of synthetic config 0's cloud on a fresh context: (cloud, graph)."""
    s = host.Synth(0)
    ctx = api.Context(s.scene)
    try:
        ctx.match_refpoints(s.seeds, device_only=True)
        cloud = ctx.fetch_device_output()
        g, _, st = ctx.replay_device()
        return cloud, g, st
    finally:
        ctx.close()


def case_a_graph():
    sa = small_scene()
    ctx = api.Context(C.byref(sa.c))
    try:
        d, held = upload_cloud(ctx, cases()["a_shared_node"])
        g, _, st = ctx.replay_device(d)
        return g, st
    finally:
        ctx.close()


if __name__ == "__main__":  # the child of the table-stress test: python replay_gpu_cases.py <out.npz>
    _, g0, st0 = config0_graph()
    ga, sta = case_a_graph()
    out = {"slots0": st0["table_slots"], "pairs0": st0["n_pairs"], "slotsa": sta["table_slots"], "pairsa": sta["n_pairs"]}
    for tag, g in (("c0", g0), ("a", ga)):
        for f in FIELDS + ARRAYS:
            out[tag + "_" + f] = g[f]
    np.savez(sys.argv[1], **out)
