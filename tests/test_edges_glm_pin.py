"""distance_point_line_sq of csrc/eg3d_edges_core.h pinned against the REFERENCE'S OWN vendored glm (external/glm 0.9.6):
glm::cross, glm::dot and the division of geometric_utilities.cpp:1003-1005, bit for bit.

The core header's host compilation is tests/glm/edges_core_driver.cpp, built at test time with the host library's
arithmetic flags. Where the reference tree is present, tests/glm/edges_glm_driver.cpp — this repository's own driver — is
compiled against that glm into a temporary directory and both run on 20 000 seeded records; the committed vectors are checked
to be what it computes. Everywhere, the core header is held to tests/golden/edges_glm_pin_v1.npz: 256 recorded inputs and the
outputs glm computed for them (data only). `python tests/test_edges_glm_pin.py` rewrites it. Values are compared as bit
patterns; NaN results only have to be NaN on both sides (as tests/test_transform_glm_pin.py). The numpy restatement of the
tests (edges_ref.distance_point_line_sq) is held to the same vectors."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLM_INC = "/root/reference/external/glm"
GLM_DRIVER = os.path.join(ROOT, "tests", "glm", "edges_glm_driver.cpp")
CORE_DRIVER = os.path.join(ROOT, "tests", "glm", "edges_core_driver.cpp")
GOLD = os.path.join(ROOT, "tests", "golden", "edges_glm_pin_v1.npz")


def have_reference():
    return os.path.isdir(os.path.join(GLM_INC, "glm"))


def build_glm_driver(directory):
    exe = os.path.join(str(directory), "edges_glm_driver")
    subprocess.check_call(["g++", "-O3", "-funroll-loops", "-std=c++11", "-w", "-I", GLM_INC, "-o", exe, GLM_DRIVER])
    return exe


def build_core_driver(directory):
    exe = os.path.join(str(directory), "edges_core_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I",
                           os.path.join(ROOT, "edgegraph3d_amd", "csrc"), "-o", exe, CORE_DRIVER])
    return exe


def run(exe, records):
    a = np.ascontiguousarray(records, np.float32).reshape(-1, 9)
    p = subprocess.run([exe], input=a.tobytes(), stdout=subprocess.PIPE, check=True)
    out = np.frombuffer(p.stdout, np.float32).copy()
    assert out.shape == (len(a),)
    return out


def cases(n, seed):
    """Seeded records (p, a, b): scene-sized coordinates, points near their line (where the test decides), far from it, lines
    of widely different lengths; then a tail of edge cases — a == b (0 / 0), p on the line, huge, tiny and denormal values,
    NaN and inf."""
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 50, (n, 3))
    d = rng.normal(0, 1, (n, 3)) * (10.0 ** rng.uniform(-3, 3, (n, 1)))
    t = rng.uniform(-0.5, 1.5, (n, 1))
    off = rng.normal(0, 1, (n, 3)) * (10.0 ** rng.uniform(-5, 1, (n, 1)))
    rec = np.concatenate([a + t * d + off, a, a + d], 1).astype(np.float32)
    rec[-1, 6:9] = rec[-1, 3:6]                        # direction 0: NaN
    rec[-2, 0:3] = rec[-2, 3:6]                        # p == a: 0
    rec[-3] = [1, 0.5, 0, 0, 0, 0, 4, 0, 0]            # the exact 0.25
    rec[-4] *= np.float32(1e18)                        # the squares overflow
    rec[-5] *= np.float32(1e-20)                       # ... and underflow
    rec[-6, 0:3] = [np.nan, 1, 2]
    rec[-7, 6:9] = [np.inf, 0, 0]
    rec[-8, 0:3] = [0.0, -0.0, 1e-42]
    rec[-9] = [3e38, -3e38, 3e38, 1, 2, 3, 4, 5, 6]
    return rec


def _same(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    eq = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(~eq)
    assert not len(bad), "%s: %d values differ from glm, first at %d: %r vs %r" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return build_core_driver(tmp_path_factory.mktemp("edges_core"))


def test_core_header_equals_glm_on_the_committed_vectors(core):
    g = np.load(GOLD)
    assert g["records_in"].shape == (256, 9) and g["records_out"].shape == (256,)
    _same(run(core, g["records_in"]), g["records_out"], "committed vectors")
    assert np.isfinite(g["records_out"][:200]).all() and np.isnan(g["records_out"][-1]) and g["records_out"][-3] == np.float32(0.25)


def test_numpy_restatement_equals_glm_on_the_committed_vectors():
    import edges_ref as er
    g = np.load(GOLD)
    got = np.array([er.distance_point_line_sq(r[0:3], r[3:6], r[6:9])[0] for r in g["records_in"]], np.float32)
    _same(got, g["records_out"], "numpy restatement")


def test_live_records_against_the_reference_glm(core, tmp_path):
    """Runs where the reference tree is; elsewhere the committed vectors above are the whole pin."""
    if not have_reference():
        return
    exe = build_glm_driver(tmp_path)
    a = cases(20000, 0xED6E5)
    _same(run(core, a), run(exe, a), "live, 20 000 records")
    g = np.load(GOLD)   # the fixture is data: regenerated from its recorded inputs it comes out identical
    _same(run(exe, g["records_in"]), g["records_out"], "fixture")


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        rec = cases(256, 0xE63D2017)
        np.savez_compressed(GOLD, records_in=rec, records_out=run(build_glm_driver(d), rec))
    print("wrote", GOLD, os.path.getsize(GOLD), "bytes")
    sys.exit(0)
