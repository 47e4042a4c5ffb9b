"""examples/json_to_ply.cpp, the reference's third tool, on a hand-written OpenMVG file of three points and three PNG images
written here: the file it writes equals the Python restatement (tests/colour_ref.py) byte for byte — without -i (white
points, no GPU), with -i ... --host (the host statement, no GPU) and, under -m gpu, with -i alone (K15 on the device). A
missing image fails the run with a message."""
import json
import subprocess

import numpy as np
import pytest

import cbuild
import colour_ref as cr
from test_colour_host import _png

SIZES = ((7, 5), (3, 2), (1, 1))   # each view its own size
POINTS = [([1.5, -2.0, 800.0], [(0, 1.25, 2.5), (2, 0.0, 0.0), (1, -0.5, 0.75)]),
          ([1e-5, 1234567.0, -0.0], [(1, 2.5, 1.0), (0, 6.5, 4.5)]),
          ([123456.7, 0.1, 3.0], [(2, 3.0, -4.0), (0, 0.0, 0.0), (0, 3.5, 3.5), (1, 1.0, 1.0)])]


def _doc():
    R = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    views = [{"key": i, "value": {"polymorphic_id": 1073741824, "ptr_wrapper": {"id": 2147483649 + i, "data": {
        "local_path": "/", "filename": "%04d.png" % i, "width": 7, "height": 5, "id_view": i, "id_intrinsic": 0, "id_pose": i}}}}
        for i in range(3)]
    extr = [{"key": i, "value": {"rotation": R, "center": [100.0 * i, 0.5, -2.25]}} for i in range(3)]
    structure = [{"key": k, "value": {"X": X, "observations": [{"key": v, "value": {"id_feat": 0, "x": [x, y]}} for v, x, y in obs]}}
                 for k, (X, obs) in enumerate(POINTS)]
    return {"sfm_data_version": "0.3", "root_path": "/data/imgs", "views": views,
            "intrinsics": [{"key": 0, "value": {"polymorphic_id": 2147483649, "polymorphic_name": "pinhole", "ptr_wrapper": {
                "id": 2147483660, "data": {"width": 7, "height": 5, "focal_length": 10.5, "principal_point": [3.0, 2.0]}}}}],
            "extrinsics": extr, "structure": structure, "control_points": []}


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("json_to_ply")
    exe = cbuild.build_caller("examples/json_to_ply.cpp", d, lib=cbuild.DEFAULT_LIB)
    json.dump(_doc(), open(d / "in.json", "w"))
    rng = np.random.default_rng(31)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in SIZES]
    (d / "imgs").mkdir()
    for i, im in enumerate(images):
        _png(d / "imgs" / ("%04d.png" % i), im.shape[1], im.shape[0], 8, 2, [im[r].ravel() for r in range(im.shape[0])])
    X = np.array([p[0] for p in POINTS], np.float32)
    off = np.concatenate([[0], np.cumsum([len(p[1]) for p in POINTS])])
    flat = [o for p in POINTS for o in p[1]]
    refused, rgb, _, _ = cr.colour(images, off, [o[0] for o in flat], [(o[1], o[2]) for o in flat])
    assert not refused and len(np.unique(rgb, axis=0)) == 3
    return exe, d, X, rgb


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_white_points_need_no_images(tool):
    exe, d, X, _ = tool
    out = _run(exe, d / "in.json", d / "white.ply")
    assert out.returncode == 0, out.stdout + out.stderr
    assert (d / "white.ply").read_bytes() == cr.ply_bytes(X)


def test_coloured_by_the_host_statement(tool):
    exe, d, X, rgb = tool
    out = _run(exe, "-i", str(d / "imgs") + "/", "--host", d / "in.json", d / "host.ply")
    assert out.returncode == 0, out.stdout + out.stderr
    assert (d / "host.ply").read_bytes() == cr.ply_bytes(X, rgb)
    assert "coloured on the host" in out.stdout


def test_a_missing_image_fails_with_a_message(tool):
    exe, d, _, _ = tool
    out = _run(exe, "-i", str(d / "nowhere") + "/", "--host", d / "in.json", d / "none.ply")
    assert out.returncode == 1 and "cannot read" in out.stderr and "0000.png" in out.stderr
    assert _run(exe, d / "in.json").returncode == 1    # the usage


@pytest.mark.gpu
def test_example_writes_the_final_cloud(tmp_path):
    """examples/edge_matcher_refpoints.cpp --ply FILE [--ply-images DIR/]: the final cloud of out.json, white and coloured
    (eg3d_colour_points on the run's context), equals the host statement on the file it wrote."""
    import ctypes as C
    import os
    from edgegraph3d_amd import _cdefs as D
    from edgegraph3d_amd import host
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "1", d])
    L = host.lib()
    h = L.eg3d_sfm_read_json((d + "/input.json").encode())
    V = L.eg3d_sfm_n_views(h)
    names = [os.path.basename(L.eg3d_sfm_image_path(h, v).decode()) for v in range(V)]
    L.eg3d_sfm_destroy(h)
    assert len(set(names)) == V and all(names)
    rng = np.random.default_rng(77)
    images = [rng.integers(0, 256, (48, 64 + v, 3), dtype=np.uint8) for v in range(V)]
    os.mkdir(d + "/imgs")
    for name, im in zip(names, images):
        _png(tmp_path / "imgs" / name, im.shape[1], im.shape[0], 8, 2, [im[r].ravel() for r in range(im.shape[0])])
    run = [exe, d + "/input.json", d + "/plgs.bin", d + "/out.json", "--all-pairs", "--ply"]
    white = subprocess.run(run + [d + "/white.ply"], capture_output=True, text=True, timeout=300)
    assert white.returncode == 0, white.stdout + white.stderr
    col = subprocess.run(run + [d + "/col.ply", "--ply-images", d + "/imgs/"], capture_output=True, text=True, timeout=300)
    assert col.returncode == 0 and "coloured" in col.stdout, col.stdout + col.stderr
    h = L.eg3d_sfm_read_json((d + "/out.json").encode())
    n = int(L.eg3d_sfm_n_points(h))
    s = D.Seeds()
    L.eg3d_sfm_seeds(h, C.byref(s))
    off = D.as_np(s.trk_off, n + 1, np.uint32)
    m = int(off[-1])
    view, xy = D.as_np(s.trk_view, m, np.int32), D.as_np(s.trk_xy, 2 * m, np.float32).reshape(m, 2)
    X = D.as_np(L.eg3d_sfm_points(h), 3 * n, np.float32).reshape(n, 3)
    L.eg3d_sfm_destroy(h)
    assert n > 0 and m > n
    rgb, _, counts = host.colour_points(images, off, view, xy, n_threads=4)
    assert counts["n_coloured"] == n
    assert open(d + "/white.ply", "rb").read() == cr.ply_bytes(X)
    assert open(d + "/col.ply", "rb").read() == cr.ply_bytes(X, rgb)


@pytest.mark.gpu
def test_coloured_on_the_device(tool):
    exe, d, X, rgb = tool
    out = _run(exe, "-i", str(d / "imgs") + "/", d / "in.json", d / "device.ply")
    assert out.returncode == 0, out.stdout + out.stderr
    assert (d / "device.ply").read_bytes() == cr.ply_bytes(X, rgb)
    assert "coloured on the device" in out.stdout
