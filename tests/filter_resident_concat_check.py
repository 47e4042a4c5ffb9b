"""Compaction of a cloud the context did NOT produce: the eg3d_concat_edgepoints of two halves computed on two
contexts (run as a script in its own process by tests/test_gpu_filter_resident.py: libeg3d_rccl.so pulls in librccl,
which must not share a process with the HIP runtime of the torch wheel that other test modules import)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgegraph3d_amd import _cdefs as D  # noqa: E402
from edgegraph3d_amd import api, host  # noqa: E402
from edgegraph3d_amd._cabi import EG3D_RCCL, bind  # noqa: E402
from edgegraph3d_amd.cloudnp import np_compact, same_cloud  # noqa: E402


def main():
    G = bind(C.CDLL(os.path.join(os.path.dirname(os.path.abspath(api.__file__)), "libeg3d_rccl.so")), EG3D_RCCL)
    s = host.Synth(2)
    a = api.Context(s.scene)
    a.upload_seeds(s.seeds)
    b = a.clone()
    h = s.n_seeds // 2
    a.match_resident(0, h, device_only=True)
    b.match_resident(h, s.n_seeds, device_only=True)
    parts = (D.DeviceEdgePoints * 2)()
    parts[0], parts[1] = a.last_device_output(), b.last_device_output()
    g = G.eg3d_gather_create(0)
    assert g
    cat = D.DeviceEdgePoints()
    assert G.eg3d_concat_edgepoints(g, 2, parts, None, C.byref(cat)) == 0
    n = int(cat.n_points)
    assert n == int(parts[0].n_points) + int(parts[1].n_points) > 0
    whole = a.fetch_device_points(cat, 0, n)
    rng = np.random.default_rng(11)
    keep = (rng.random(n) < 0.6).astype(np.uint8)
    Xn = rng.standard_normal((n, 3)).astype(np.float32)
    out = a.compact_device(cat, a.upload(keep), a.upload(Xn), 4)
    got = a.fetch_device_points(out, 0, int(out.n_points))
    want = np_compact(whole, keep, Xn, 4)
    assert 0 < want["n_points"] < n
    bad = same_cloud(got, want)
    assert bad is None, bad
    G.eg3d_gather_destroy(g)
    b.close()
    a.close()
    print("CONCAT-COMPACT-OK %d -> %d points" % (n, want["n_points"]))


if __name__ == "__main__":
    main()
