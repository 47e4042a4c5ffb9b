"""The FP32 half of include/eg3d_host_transform.h pinned against the REFERENCE'S OWN vendored glm (external/glm 0.9.6):
vec4 * mat4 and the division (transform_3d_point), glm::inverse(mat4), inverse(M) * rt4x4 and the e * K4 product
(update_camera_transform), bit for bit. The FP64 fit is NOT pinned (Eigen is not available: DESIGN.md 3).

Where the reference tree is present, tests/glm/transform_glm_driver.cpp — this repository's own driver — is compiled
against that glm at test time into a temporary directory and run on 10 000 seeded records; the committed vectors are
checked to be what it computes. Everywhere, the host statement is held to tests/golden/transform_glm_pin_v1.npz: 64
recorded inputs and the outputs glm computed for them (data only). `python tests/test_transform_glm_pin.py` rewrites it.
Values are compared as bit patterns; NaN results only have to be NaN on both sides (as tests/test_glm_pin.py)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLM_INC = "/root/reference/external/glm"
DRIVER_SRC = os.path.join(ROOT, "tests", "glm", "transform_glm_driver.cpp")
GOLD = os.path.join(ROOT, "tests", "golden", "transform_glm_pin_v1.npz")
N_IN, N_OUT = 34, 51


def have_reference():
    return os.path.isdir(os.path.join(GLM_INC, "glm"))


def build_driver(directory):
    exe = os.path.join(str(directory), "transform_glm_driver")
    subprocess.check_call(["g++", "-O3", "-funroll-loops", "-std=c++11", "-w", "-I", GLM_INC, "-o", exe, DRIVER_SRC])
    return exe


def run_glm(exe, records):
    a = np.ascontiguousarray(records, np.float32)
    p = subprocess.run([exe], input=a.tobytes(), stdout=subprocess.PIPE, check=True)
    return np.frombuffer(p.stdout, np.float32).reshape(len(a), N_OUT).copy()


def cases(n, seed):
    """Seeded records: fitted-similarity-like matrices with DTU-like cameras and points, every fourth matrix a general
    one (projective last row), then a tail of edge cases — a singular matrix, huge and tiny entries, NaN and inf points."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, N_IN), np.float32)
    for i in range(n):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        M = np.eye(4)
        M[:3, :3] = rng.uniform(0.1, 10) * Q
        M[:3, 3] = rng.normal(0, 300, 3)
        if i % 4 == 3:
            M = rng.normal(0, 1, (4, 4)) * rng.choice([1e-3, 1, 1e3])
        R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        a[i, :16] = M.reshape(16)
        a[i, 16:25] = R.reshape(9)
        a[i, 25:28] = rng.normal(0, 500, 3)
        a[i, 28:31] = [rng.uniform(500, 4000), rng.uniform(300, 1300), rng.uniform(200, 900)]
        a[i, 31:34] = rng.normal(0, 200, 3)
    a[-1, :16] = 0                                # singular: 1 / 0
    a[-2, 31:34] = [np.nan, 1.0, 2.0]
    a[-3, 31:34] = [np.inf, -1.0, 2.0]
    a[-4, :16] *= np.float32(1e9)                 # cofactors overflow
    a[-5, :16] *= np.float32(1e-9)
    a[-6, 31:34] = [0.0, -0.0, 1e-42]             # a denormal coordinate
    a[-7, 12:16] = [0.0, 0.0, 0.0, 0.0]           # h[3] == 0: the division by zero
    a[-8, 31:34] = [3e38, 3e38, -3e38]
    return a


def host_statement(records):
    """what the library computes for the same records, laid out like the driver's output"""
    from edgegraph3d_amd import host
    a = np.ascontiguousarray(records, np.float32)
    out = np.zeros((len(a), N_OUT), np.float32)
    for i, r in enumerate(a):
        M = r[:16].reshape(4, 4)
        T = M.astype(np.float64)                  # (a float widens exactly: the library's conversion gives M back)
        out[i, :3] = host.transform_points(T, r[31:34])
        inv = host.glm_inverse4(M)
        out[i, 3:19] = inv.reshape(16)
        E = np.zeros((4, 4), np.float32)
        E[:3, :3], E[:3, 3], E[3, 3] = r[16:25].reshape(3, 3), r[25:28], 1
        K = np.zeros((4, 4), np.float32)
        K[0, 0] = K[1, 1] = r[28]
        K[0, 2], K[1, 2], K[2, 2] = r[29], r[30], 1
        e = host.glm_mul4(inv, E)
        out[i, 19:35] = e.reshape(16)
        out[i, 35:51] = host.glm_mul4(e, K).reshape(16)
    return out


def _same(got, want, what):
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    eq = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    bad = np.argwhere(~eq)
    assert not len(bad), "%s: %d values differ from glm, first at %s: %r vs %r" % (
        what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def test_host_statement_equals_glm_on_the_committed_vectors():
    g = np.load(GOLD)
    assert g["records_in"].shape == (64, N_IN) and g["records_out"].shape == (64, N_OUT)
    _same(host_statement(g["records_in"]), g["records_out"], "committed vectors")
    assert np.isfinite(g["records_out"][:40]).all() and not np.isfinite(g["records_out"][-8:]).all()


def test_transform_cameras_is_made_of_the_pinned_pieces():
    """eg3d_host_transform_cameras against the recorded e and P of the same records (finite matrices only: the call
    refuses the others)"""
    from edgegraph3d_amd import host
    g = np.load(GOLD)
    n = 0
    for r, w in zip(g["records_in"], g["records_out"]):
        if not np.isfinite(r[:16]).all():
            continue
        T = r[:16].reshape(4, 4).astype(np.float64)
        own_centre = bool(np.isfinite(r[31:34]).all())
        C3 = r[31:34] if own_centre else np.float32([1, 2, 3])
        R, C, t, P = host.transform_cameras(T, r[28:31], r[16:25], C3, r[25:28])
        e = w[19:35].reshape(4, 4)
        _same(R.reshape(3, 3), e[:3, :3], "rotation")
        _same(t.reshape(3), e[:3, 3], "translation")
        _same(P.reshape(16), w[35:51], "cameraMatrix")
        if own_centre:
            _same(C.reshape(3), w[:3], "center")
        n += 1
    assert n == 64


def test_live_ten_thousand_records_against_the_reference_glm(tmp_path):
    """Runs where the reference tree is; elsewhere the committed vectors above are the whole pin."""
    if not have_reference():
        return
    exe = build_driver(tmp_path)
    a = cases(10000, 0x7A16)
    _same(host_statement(a), run_glm(exe, a), "live, 10 000 records")
    g = np.load(GOLD)   # the fixture is data: regenerated from its recorded inputs it comes out identical
    _same(run_glm(exe, g["records_in"]), g["records_out"], "fixture")


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        rec = cases(64, 0xE63D2016)
        np.savez_compressed(GOLD, records_in=rec, records_out=run_glm(build_driver(d), rec))
    print("wrote", GOLD, os.path.getsize(GOLD), "bytes")
    sys.exit(0)
