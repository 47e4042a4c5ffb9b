"""Child process of tests/test_gpu_nearest.py::test_the_device_outputs_feed_compact_device. torch and the product library
share one HIP runtime only when torch initialises the device first (bench.py's order), which a pytest process that has
already loaded the library cannot arrange; so the chain runs here: nearest_device writes d2 / nn into torch tensors, the
mask d2 < t * t is computed by torch on the device, and compact_device keeps exactly n_below points. EG3D_LIB (inherited)
selects the library. Prints one line "OK <n_points> <n_below>" and exits 0, or raises."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    torch.cuda.init()
    from edgegraph3d_amd import api, host
    F = np.float32
    s = host.Synth(1)
    ctx = api.Context(s.scene)
    ctx.match_refpoints(s.seeds, device_only=True)
    X = ctx.fetch_device_output()["X"]
    n = len(X)
    rng = np.random.default_rng(78)
    md = float(F(0.01 * float(np.ptp(X[np.isfinite(X).all(axis=1)], axis=0).max())))
    t = float(F(0.25 * md))
    ref = (X[::2] + rng.normal(0, 0.2 * md, X[::2].shape)).astype(F)
    dev = torch.device("cuda", ctx.device)
    d2 = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
    nn = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    with ctx.cloud_index(X=ref, cell=md) as index:
        r = ctx.nearest_device(index, md, thresholds=(t,), to_host=False, d2=d2.data_ptr(), nn=nn.data_ptr())
    mask = (d2 < float(F(t) * F(t))).to(torch.uint8)        # t * t in FP32, exact as a double; the mask stays on the device
    torch.cuda.synchronize(dev)
    n_below = r["stats"]["n_below"][0]
    assert int(mask.sum().item()) == n_below and 0 < n_below < n, (int(mask.sum().item()), n_below, n)
    want_d2, want_nn, _ = host.cloud_nearest(ref, X, md, thresholds=(t,))
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), want_d2.view(np.uint32))
    assert np.array_equal(nn.cpu().numpy().view(np.uint32), want_nn)
    out = ctx.compact_device(ctx.last_device_output(), keep=mask.data_ptr())
    assert int(out.n_points) == n_below, (int(out.n_points), n_below)
    kept = ctx.fetch_device_points(out, 0, n_below)["X"]
    assert np.array_equal(kept.view(np.uint32), X[mask.cpu().numpy() != 0].view(np.uint32))
    ctx.close()
    print("OK %d %d" % (n, n_below))


if __name__ == "__main__":
    main()
