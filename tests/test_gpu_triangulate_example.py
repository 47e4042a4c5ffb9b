"""-m gpu: K14 as C++ callers reach it. compute_3d_point_coords of include/eg3d_refapi.hpp (tests/refapi/triangulate_check.cpp:
the batched overload and the reference's one-point signature, on a private context built from the cameras alone) gives the
bits of the host statement on the seed tracks of config 1; examples/edge_matcher_refpoints.cpp --triangulate-refpoints
prints the counts Context.triangulate returns, and prints nothing of the kind without the flag."""
import re
import subprocess

import numpy as np
import pytest

import cbuild
from edgegraph3d_amd import api, host

pytestmark = pytest.mark.gpu


def _want(s, form):
    off, view, xy = s.seeds_np()
    off = np.concatenate([off, [off[-1] + 1]]).astype(np.uint32)   # + the short track: the first observation of track 0
    view, xy = np.concatenate([view, view[:1]]), np.concatenate([xy, xy[:1]])
    return host.triangulate(s.scene_np()["cam_P"], off, view, xy, mode=0, dlt_rows=form, n_threads=4)


def test_refapi_compute_3d_point_coords(eg3d_form, tmp_path):
    exe = cbuild.build_caller("tests/refapi/triangulate_check.cpp", tmp_path)
    out = subprocess.run([exe, "1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    X, valid, flags = _want(host.Synth(1), eg3d_form)
    n = len(valid)
    bits = X.view(np.uint32)
    rows = [l.split() for l in lines[:n]]
    assert [int(r[0]) for r in rows] == valid.tolist() and [int(r[1]) for r in rows] == flags.tolist()
    assert [[int(t, 16) for t in r[2:]] for r in rows] == bits.tolist()
    assert valid[:-1].all() and not valid[-1] and flags[-1] == api.TRI_FLAG_SHORT
    assert lines[n] == "single 4"
    seven = int(np.float32(7).view(np.uint32))
    for k, i in enumerate((0, 1, 2, n - 1)):   # the one-point signature: the point is assigned only when valid
        got = lines[n + 1 + k].split()
        assert int(got[0]) == valid[i]
        assert [int(t, 16) for t in got[1:]] == (bits[i].tolist() if valid[i] else [seven] * 3)


def test_example_flag_prints_the_counts(eg3d_form, tmp_path):
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "1", d])
    s = host.Synth(1)
    ctx = api.Context(s.scene)
    st = ctx.triangulate(*s.seeds_np())[3]
    ctx.close()
    out = subprocess.run([exe, d + "/input.json", d + "/plgs.bin", d + "/out.json", "--all-pairs", "--triangulate-refpoints"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"reference-point tracks: (\d+) of (\d+) triangulate from their own observations \((\d+) short, (\d+) with", out.stdout)
    assert m, out.stdout
    assert [int(g) for g in m.groups()] == [st["n_valid"], s.n_seeds, st["n_short"], st["n_degenerate"]]
    assert st["n_valid"] > 0
    plain = subprocess.run([exe, d + "/input.json", d + "/plgs.bin", d + "/out2.json", "--all-pairs"], capture_output=True,
                           text=True, timeout=300)
    assert plain.returncode == 0 and "reference-point tracks" not in plain.stdout   # off by default
    assert open(d + "/out.json", "rb").read() == open(d + "/out2.json", "rb").read()   # and the flag changes nothing else
