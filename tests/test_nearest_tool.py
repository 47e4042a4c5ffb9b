"""examples/compare_clouds.cpp and the --compare flag of examples/edge_matcher_refpoints.cpp. Without a GPU: the tool's --host
route prints the figures host.compare_clouds gives. -m gpu: the device route prints the identical text, and --compare on the
synthetic scene prints the figures of the Python host route on the run's output."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cbuild
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import host

F = np.float32
MD, TH = 0.02, (0.01, 0.005)


def _clouds(d):
    rng = np.random.default_rng(1)
    A = rng.uniform(0, 1, (3000, 3)).astype(F)
    B = (A[::2] + rng.normal(0, 0.004, (1500, 3))).astype(F)
    host.write_ply(d + "/a.ply", A)
    host.write_ply(d + "/b.ply", B)
    return host.read_ply_points(d + "/a.ply"), host.read_ply_points(d + "/b.ply")      # (what the tool reads: six digits)


def _args(d):
    return [d + "/a.ply", d + "/b.ply", "--max-dist", str(MD)] + [x for t in TH for x in ("--threshold", str(t))]


def _expected(A, B):
    c = host.compare_clouds(A, B, MD, thresholds=TH)
    lines = []
    for name, s in (("accuracy (A -> B)", c["accuracy"]), ("completeness (B -> A)", c["completeness"])):
        lines.append("%s: %d points (%d not finite), %d within %g, mean %.9g, median %.9g" % (
            name, s["n_queries"], s["n_nonfinite"], s["n_within"], float(F(MD)), s["mean"], s["median"]))
        used = s["n_queries"] - s["n_dropped"] - s["n_nonfinite"]
        lines += ["  below %g: %d (%.4f%%)" % (float(F(t)), b, 100.0 * b / used) for t, b in zip(TH, s["n_below"])]
    return "\n".join(lines) + "\n"


def test_the_tool_on_the_host_prints_the_python_figures(tmp_path):
    exe = cbuild.build_caller("examples/compare_clouds.cpp", tmp_path)
    d = str(tmp_path)
    A, B = _clouds(d)
    out = subprocess.run([exe] + _args(d) + ["--host"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout == _expected(A, B)
    assert "within 0.02, mean 0.00" in out.stdout
    # refusals: no reach, a file that is no PLY
    assert subprocess.run([exe, d + "/a.ply", d + "/b.ply", "--host"], capture_output=True).returncode == 1
    (tmp_path / "bad.ply").write_bytes(b"ply\nformat binary_big_endian 1.0\nend_header\n")
    bad = subprocess.run([exe, d + "/a.ply", d + "/bad.ply", "--max-dist", "0.02", "--host"], capture_output=True, text=True)
    assert bad.returncode == 1 and "big-endian" in bad.stderr
    far = subprocess.run([exe] + _args(d) + ["--host", "--cell", "0.01"], capture_output=True, text=True)
    assert far.returncode == 1 and "max_dist" in far.stderr


@pytest.mark.gpu
def test_the_tool_on_the_device_prints_the_same_text(eg3d_form, tmp_path):
    exe = cbuild.build_caller("examples/compare_clouds.cpp", tmp_path)
    d = str(tmp_path)
    A, B = _clouds(d)
    dev = subprocess.run([exe] + _args(d), capture_output=True, text=True, timeout=120)
    assert dev.returncode == 0, dev.stdout + dev.stderr
    assert dev.stdout == _expected(A, B)


@pytest.mark.gpu
def test_compare_flag_of_the_example(eg3d_form, tmp_path):
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "1", d])
    common = [d + "/input.json", d + "/plgs.bin"]
    plain = subprocess.run([exe] + common + [d + "/out.json", "--all-pairs"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "compare:" not in plain.stdout, plain.stdout + plain.stderr
    L = host.lib()
    h = L.eg3d_sfm_read_json(os.fsencode(d + "/out.json"))
    n = int(L.eg3d_sfm_n_points(h))
    X = D.as_np(L.eg3d_sfm_points(h), 3 * n, F).reshape(n, 3)
    L.eg3d_sfm_destroy(h)
    fin = np.isfinite(X).all(axis=1)
    md = float(F(0.02 * float(np.ptp(X[fin], axis=0).max())))
    ref = (X[fin][::2] + np.random.default_rng(2).normal(0, 0.2 * md, X[fin][::2].shape)).astype(F)
    host.write_ply(d + "/ref.ply", ref)
    ref = host.read_ply_points(d + "/ref.ply")
    out = subprocess.run([exe] + common + [d + "/out2.json", "--all-pairs", "--compare", d + "/ref.ply", "--compare-max-dist", repr(md)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(d + "/out.json", "rb").read() == open(d + "/out2.json", "rb").read()   # the flag changes nothing else
    want = host.compare_clouds(X, ref, md)
    for side in ("accuracy", "completeness"):
        m = re.search(r"compare: %s: (\d+) points, (\d+) within \S+ mean (\S+), median (\S+)" % side, out.stdout)
        assert m, out.stdout
        s = want[side]
        assert [int(m.group(1)), int(m.group(2))] == [s["n_queries"], s["n_within"]] and s["n_within"] > 0
        assert m.group(3) == "%.9g" % s["mean"] and m.group(4) == "%.9g" % s["median"]
