"""examples/coordinate_system_transform.cpp, the reference's fourth tool, on a hand-written OpenMVG file of six cameras (one
of them without a pose) and a poses file written here: with --host (no GPU) the JSON it writes parses, its cameras and
points equal the Python composition of the host calls value for value, and the lines the reference prints are there. Under
-m gpu the same run without --host (K16 on the device) writes the same bytes."""
import json
import subprocess

import numpy as np
import pytest

import cbuild
from edgegraph3d_amd import host

V, NULL = 6, 3
FPP = (10.5, 3.0, 2.0)


def _rig():
    rng = np.random.default_rng(58)
    R = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(V)]).astype(np.float32)
    C = (rng.normal(size=(V, 3)) * 3).astype(np.float32)
    R[NULL], C[NULL] = 0, 0
    X = (rng.normal(size=(40, 3)) * 2).astype(np.float32)
    # the target frame: a similarity of the centres plus a little noise, so that the error after is small but not zero
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 2] = -Q[:, 2]
    poses = 2.5 * C.astype(np.float64) @ Q.T + [10, -20, 30] + rng.normal(size=(V, 3)) * 1e-3
    poses[NULL] = [7e8, 7e8, 7e8]   # read and dropped
    return R, C, X, poses


def _doc(R, C, X):
    views = [{"key": i, "value": {"polymorphic_id": 1073741824, "ptr_wrapper": {"id": 2147483649 + i, "data": {
        "local_path": "/", "filename": "%04d.png" % i, "width": 7, "height": 5, "id_view": i, "id_intrinsic": 0, "id_pose": i}}}}
        for i in range(V)]
    extr = [{"key": i, "value": {"rotation": [[float(x) for x in row] for row in R[i]], "center": [float(x) for x in C[i]]}}
            for i in range(V)]
    structure = [{"key": k, "value": {"X": [float(x) for x in p], "observations": [
        {"key": (k + j) % V, "value": {"id_feat": 0, "x": [1.5 + j, 2.25]}} for j in range(2)]}} for k, p in enumerate(X)]
    return {"sfm_data_version": "0.3", "root_path": "/data/imgs", "views": views,
            "intrinsics": [{"key": 0, "value": {"polymorphic_id": 2147483649, "polymorphic_name": "pinhole", "ptr_wrapper": {
                "id": 2147483660, "data": {"width": 7, "height": 5, "focal_length": FPP[0], "principal_point": list(FPP[1:])}}}}],
            "extrinsics": extr, "structure": structure, "control_points": []}


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("coordinate_system_transform")
    exe = cbuild.build_caller("examples/coordinate_system_transform.cpp", d, lib=cbuild.DEFAULT_LIB)
    R, C, X, poses = _rig()
    json.dump(_doc(R, C, X), open(d / "in.json", "w"))
    (d / "poses.txt").write_text("".join("%r %r %r\n" % tuple(float(x) for x in p) for p in poses))
    # the Python composition of the host calls
    fpp = np.tile(np.float32(FPP), (V, 1))
    t, P = np.zeros((V, 3), np.float32), np.zeros((V, 16), np.float32)
    import ctypes as Ct
    from edgegraph3d_amd import _cdefs as D
    Rf, Cf = np.ascontiguousarray(R.reshape(V, 9)), np.ascontiguousarray(C)
    assert host.lib().eg3d_host_camera_model(V, D.np_ptr(fpp, Ct.c_float), D.np_ptr(Rf, Ct.c_float), D.np_ptr(Cf, Ct.c_float),
                                             D.np_ptr(t, Ct.c_float), D.np_ptr(P, Ct.c_float)) == 0
    mask = host.null_cameras(Rf, Cf)
    assert mask.tolist() == [int(v == NULL) for v in range(V)]
    target = host.read_camera_poses(str(d / "poses.txt"), V)
    assert (target == poses).all()
    T, st = host.similarity_fit(Cf.astype(np.float64), target, mask)
    R2, C2, t2, P2 = host.transform_cameras(T, fpp, Rf, Cf, t)
    want = {"T": T, "R": R2, "C": C2, "t": t2, "P": P2, "X": host.transform_points(T, X), "before": host.camera_errors(Cf, target, mask),
            "after": host.camera_errors(C2, target, mask), "scale": st["scale"]}
    # the same rig as the raw file tests/refapi/transform_check.cpp reads
    np.concatenate([np.float32([V, len(X)]), np.concatenate([fpp, Rf, Cf, t], axis=1).reshape(-1), X.reshape(-1)]).astype(
        np.float32).tofile(str(d / "rig.bin"))
    return exe, d, want


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _check_output(path, want):
    doc = json.load(open(path))
    assert [e["key"] for e in doc["extrinsics"]] == list(range(V))
    R = np.float32([e["value"]["rotation"] for e in doc["extrinsics"]]).reshape(V, 9)
    C = np.float32([e["value"]["center"] for e in doc["extrinsics"]])
    X = np.float32([p["value"]["X"] for p in doc["structure"]])
    assert (R.view(np.uint32) == want["R"].view(np.uint32)).all()
    assert (C.view(np.uint32) == want["C"].view(np.uint32)).all()
    assert (X.view(np.uint32) == want["X"].view(np.uint32)).all()
    assert not R[NULL].any() and not C[NULL].any()          # the camera without a pose is written as it was read
    assert [len(p["value"]["observations"]) for p in doc["structure"]] == [2] * len(X)
    assert doc["views"][2]["value"]["ptr_wrapper"]["data"]["filename"] == "0002.png" and doc["sfm_data_version"] == "0.3"


def _check_lines(out, want):
    lines = out.stdout.splitlines()
    assert "Ignoring camera %d in computing the Umeyama transformation" % NULL in lines
    k = lines.index("T:")
    rows = np.array([[float(x) for x in lines[k + 1 + r].split()] for r in range(4)])
    assert np.abs(rows - want["T"]).max() <= 1e-5 * np.abs(want["T"]).max()      # printed with 6 significant digits
    assert len({len(l) for l in lines[k + 1:k + 5]}) == 1                          # columns aligned
    assert lines[k + 5] == "Camera position errors before: %g" % want["before"]
    assert "Camera position errors after: %g" % want["after"] in lines
    assert float(want["after"]) < 0.01 < 1 < float(want["before"])


def test_host_run_equals_the_composition_of_the_host_calls(tool):
    exe, d, want = tool
    out = _run(exe, "--host", d / "in.json", d / "poses.txt", d / "host.json")
    assert out.returncode == 0, out.stdout + out.stderr
    _check_output(d / "host.json", want)
    _check_lines(out, want)
    assert "transformed on the host" in out.stdout


def test_bad_inputs_fail_with_a_message(tool):
    exe, d, _ = tool
    (d / "short.txt").write_text("1 2 3\n4 5 6\n")
    out = _run(exe, "--host", d / "in.json", d / "short.txt", d / "none.json")
    assert out.returncode == 1 and "fewer than three numbers per camera" in out.stderr and not (d / "none.json").exists()
    out = _run(exe, "--host", d / "in.json", d / "missing.txt", d / "none.json")
    assert out.returncode == 1 and "cannot be opened" in out.stderr
    out = _run(exe, "--host", d / "missing.json", d / "poses.txt", d / "none.json")
    assert out.returncode == 1 and "cannot read" in out.stderr
    assert _run(exe, d / "in.json").returncode == 1    # the usage


def _seam(d, want, *mode):
    """tests/refapi/transform_check.cpp: include/eg3d_transform_coordinate_system.hpp on the same rig"""
    exe = cbuild.build_caller("tests/refapi/transform_check.cpp", d, lib=cbuild.DEFAULT_LIB)
    out = _run(exe, d / "rig.bin", d / "poses.txt", d / "seam.bin", *mode)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.fromfile(str(d / "seam.bin"), np.float32)
    cams, X = got[:31 * V].reshape(V, 31), got[31 * V:].reshape(-1, 3)
    for name, a in (("R", cams[:, :9]), ("C", cams[:, 9:12]), ("t", cams[:, 12:15]), ("P", cams[:, 15:31]), ("X", X)):
        assert (np.ascontiguousarray(a).view(np.uint32) == want[name].view(np.uint32)).all(), name
    _check_lines(out, want)
    return exe


def test_cpp_seam_equals_the_host_calls(tool):
    _, d, want = tool
    exe = _seam(d, want)
    out = _run(exe, d / "rig.bin", d / "short.txt", d / "none.bin")      # (short.txt: written by the test above, or missing)
    assert out.returncode == 4 and "Eg3dError" in out.stderr


@pytest.mark.gpu
def test_cpp_seam_on_the_device(tool):
    _, d, want = tool
    _seam(d, want, "device")


@pytest.mark.gpu
def test_example_aligns_the_final_cloud(tmp_path):
    """examples/edge_matcher_refpoints.cpp --align FILE --ply FILE: out.json stays in the reconstruction's frame, the PLY
    file holds its points through the similarity fitted to FILE's centres (the host statement on the file it wrote)."""
    import ctypes as C
    import colour_ref as cr
    from edgegraph3d_amd import _cdefs as D
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "1", d])
    L = host.lib()
    h = L.eg3d_sfm_read_json((d + "/input.json").encode())
    n_views = L.eg3d_sfm_n_views(h)
    centres, mask = np.zeros((n_views, 3)), np.zeros(n_views, np.uint8)
    assert L.eg3d_sfm_camera_centres(h, D.np_ptr(centres, C.c_double), D.np_ptr(mask, C.c_uint8)) == 0 and not mask.any()
    L.eg3d_sfm_destroy(h)
    target = 3.0 * centres[:, [1, 2, 0]] + [5.0, 6.0, -7.0]        # a rotation (an even permutation), a scale, a shift
    (tmp_path / "poses.txt").write_text("".join("%r %r %r\n" % tuple(float(x) for x in p) for p in target))
    run = subprocess.run([exe, d + "/input.json", d + "/plgs.bin", d + "/out.json", "--all-pairs", "--align", d + "/poses.txt", "--ply",
                          d + "/aligned.ply"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "align: %d cameras, scale 3" % n_views in run.stdout, run.stdout + run.stderr
    h = L.eg3d_sfm_read_json((d + "/out.json").encode())
    n = int(L.eg3d_sfm_n_points(h))
    X = D.as_np(L.eg3d_sfm_points(h), 3 * n, np.float32).reshape(n, 3).copy()
    L.eg3d_sfm_destroy(h)
    T, st = host.similarity_fit(centres, target)
    assert n > 0 and abs(st["scale"] - 3.0) < 1e-9 and not st["reflection"]
    assert open(d + "/aligned.ply", "rb").read() == cr.ply_bytes(host.transform_points(T, X))


@pytest.mark.gpu
def test_device_run_writes_the_same_bytes(tool):
    exe, d, want = tool
    ref = _run(exe, "--host", d / "in.json", d / "poses.txt", d / "host2.json")
    out = _run(exe, d / "in.json", d / "poses.txt", d / "device.json")
    assert ref.returncode == 0 and out.returncode == 0, out.stdout + out.stderr
    assert (d / "device.json").read_bytes() == (d / "host2.json").read_bytes()
    _check_output(d / "device.json", want)
    _check_lines(out, want)
    assert "transformed on the device" in out.stdout
