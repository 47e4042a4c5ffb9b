"""-m gpu: examples/edge_matcher_refpoints.cpp --edges FILE [--edges-tol T] on the synthetic scene writes the bytes the Python
route writes from the same input files: the scene as the tool assembles it (the JSON's cameras and tracks, the polyline
graphs, analytic fundamental matrices for all pairs), match_refpoints(device_only) -> replay_device -> edge_chains_device ->
host.write_ply_edges. Without the flag the tool writes no such file and its JSON is the same."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cbuild
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host

pytestmark = pytest.mark.gpu


def _python_route(d, tol, out_path, target=None):
    """target: the camera centres of --align, or None. With it the vertices are the nodes' positions through the fitted
    similarity (the host statement of the point transform)."""
    L = host.lib()
    sfm = L.eg3d_sfm_read_json(os.fsencode(d + "/input.json"))
    plg = L.eg3d_plg_read(os.fsencode(d + "/plgs.bin"))
    assert sfm and plg
    try:
        sc = D.Scene()
        C.memmove(C.byref(sc), L.eg3d_plg_scene(plg), C.sizeof(sc))
        V = L.eg3d_sfm_n_views(sfm)
        assert sc.n_views == V
        F, Fv = np.zeros(V * V * 9), np.zeros(V * V, np.uint8)
        assert L.eg3d_sfm_analytic_F(sfm, D.np_ptr(F, C.c_double), D.np_ptr(Fv, C.c_uint8)) == 0
        sc.cam_P, sc.F, sc.F_valid = L.eg3d_sfm_cam_P(sfm), D.np_ptr(F, C.c_double), D.np_ptr(Fv, C.c_uint8)
        seeds = D.Seeds()
        assert L.eg3d_sfm_seeds(sfm, C.byref(seeds)) == 0
        ctx = api.Context(C.pointer(sc))
        try:
            ctx.match_refpoints(C.pointer(seeds), device_only=True)
            g, _, _ = ctx.replay_device()
            ch = ctx.edge_chains_device(max_dist=tol)
            assert er_same(ch, host.edge_chains(g, tol))
            X = g["node_X"]
            if target is not None:
                centres, mask = np.zeros((V, 3)), np.zeros(V, np.uint8)
                assert L.eg3d_sfm_camera_centres(sfm, D.np_ptr(centres, C.c_double), D.np_ptr(mask, C.c_uint8)) == 0
                T, _ = host.similarity_fit(centres, target, mask)
                X = host.transform_points(T, X)
            host.write_ply_edges(out_path, ch, X)
            return ch["stats"]
        finally:
            ctx.close()
    finally:
        L.eg3d_plg_destroy(plg)
        L.eg3d_sfm_destroy(sfm)


def er_same(a, b):
    import edges_ref as er
    return er.difference(a, b) is None


def test_edges_flag_writes_what_the_python_route_writes(eg3d_form, tmp_path):
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "1", d])
    common = [d + "/input.json", d + "/plgs.bin"]
    for tol, flags in ((0.01, []), (0.25, ["--edges-tol", "0.25"])):
        ply = "%s/edges_%g.ply" % (d, tol)
        out = subprocess.run([exe] + common + [d + "/out.json", "--all-pairs", "--edges", ply] + flags, capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        want = "%s/want_%g.ply" % (d, tol)
        st = _python_route(d, tol, want)
        got = open(ply, "rb").read()
        assert got == open(want, "rb").read(), tol
        m = re.search(r"edge model: (\d+) nodes, (\d+) polylines -> (\d+) chains \((\d+) rings, (\d+) loops dropped\), longest (\d+) "
                      r"vertices; (\d+) vertices -> (\d+) kept", out.stdout)
        assert m, out.stdout
        assert [int(x) for x in m.groups()[2:]] == [st[k] for k in ("n_chains", "n_rings", "n_loops_dropped", "longest_chain",
                                                                    "n_vertices_in", "n_vertices_kept")]
        assert st["n_chains"] > 0 and got.startswith(b"ply\nformat ascii 1.0\nelement vertex ") and b"element edge " in got
    # --align: the same model, its vertices in the target frame (a rotation, a scale, a shift of the input's camera centres)
    L = host.lib()
    h = L.eg3d_sfm_read_json(os.fsencode(d + "/input.json"))
    V = L.eg3d_sfm_n_views(h)
    centres, mask = np.zeros((V, 3)), np.zeros(V, np.uint8)
    assert L.eg3d_sfm_camera_centres(h, D.np_ptr(centres, C.c_double), D.np_ptr(mask, C.c_uint8)) == 0 and not mask.any()
    L.eg3d_sfm_destroy(h)
    target = 3.0 * centres[:, [1, 2, 0]] + [5.0, 6.0, -7.0]
    (tmp_path / "poses.txt").write_text("".join("%r %r %r\n" % tuple(float(x) for x in p) for p in target))
    out = subprocess.run([exe] + common + [d + "/out3.json", "--all-pairs", "--align", d + "/poses.txt", "--edges", d + "/aligned.ply"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "aligned)" in out.stdout, out.stdout + out.stderr
    _python_route(d, 0.01, d + "/want_aligned.ply", target)
    aligned = open(d + "/aligned.ply", "rb").read()
    assert aligned == open(d + "/want_aligned.ply", "rb").read()
    assert aligned != open("%s/edges_%g.ply" % (d, 0.01), "rb").read()
    plain = subprocess.run([exe] + common + [d + "/out2.json", "--all-pairs"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "edge model" not in plain.stdout
    assert open(d + "/out.json", "rb").read() == open(d + "/out2.json", "rb").read()   # the flag changes nothing else
