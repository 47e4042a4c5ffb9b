"""Single-rank check of include/eg3d_rccl_claims.h (run as a script in its OWN process by tests/test_gpu_dedup_phases.py:
/opt/rocm's librccl must not share a process with the HIP/HSA runtime bundled in the torch wheel, which other test modules
import). A communicator of one rank: the minimum all-reduce of the claim map, in several pieces with a partial last one,
leaves the map as it was; the scan of the point counts gives base 0; and the composition a C host makes — exscan, claim,
all-reduce, keep, filter, threshold, compact, gather — gives eg3d_dedup_resident(with_filter = 1) of the same cloud, all
seven arrays. Then the same through distributed.dedup_filter_then_gather."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgegraph3d_amd import _cdefs as D  # noqa: E402
from edgegraph3d_amd import api, host  # noqa: E402
from edgegraph3d_amd.cloudnp import same_cloud  # noqa: E402
from edgegraph3d_amd.distributed import RcclCloudGather, dedup_filter_then_gather, gather_lib, observation_threshold  # noqa: E402

MSE = 2.25


def main():
    G = gather_lib()
    rg = RcclCloudGather(None, 1, 0, 0)   # one communicator of one rank (and one gather) for the whole check
    comm, g = rg.comm, rg.g
    s = host.Synth(1)
    ctx = api.Context(s.scene)
    ctx.upload_seeds(s.seeds)
    ctx.match_resident(0, s.n_seeds, device_only=True)
    local = ctx.last_device_output()
    n = int(local.n_points)
    assert local.complete == 1 and n > 1000
    want, _, st = ctx.dedup_resident(with_filter=True, gn_max_mse=MSE)
    assert 0 < want["n_points"] < st["n_dedup_kept"] < n
    # ---- the two exchanges on a communicator of one rank
    base, total = C.c_uint64(7), C.c_uint64(7)
    assert G.eg3d_exscan_points(comm, 1, 0, None, n, C.byref(base), C.byref(total)) == 0
    assert base.value == 0 and total.value == n
    assert G.eg3d_exscan_points(comm, 1, 0, None, 2**32 - 1, None, None) == -1      # the run would outgrow 32-bit indices
    ctx.dedup_claim(local, base.value, reset=True)
    ptr, n_cells = ctx.dedup_claims()
    before = ctx.fetch_dedup_claims()
    assert (before != 0xFFFFFFFF).any()
    piece = 4 * (n_cells // 3 - 5)          # three whole pieces and a partial fourth
    assert 0 < n_cells * 4 % piece < piece and n_cells * 4 // piece == 3
    assert G.eg3d_allreduce_claims(comm, 1, 0, None, C.c_void_p(ptr), n_cells, 1, piece) == 0
    assert np.array_equal(ctx.fetch_dedup_claims(), before)
    assert G.eg3d_allreduce_claims(comm, 1, 0, None, C.c_void_p(ptr), n_cells, 1, 0) == 0   # (one piece)
    assert np.array_equal(ctx.fetch_dedup_claims(), before)
    # the agreement round: a rank without a usable map makes the call return before any payload moves
    assert G.eg3d_allreduce_claims(comm, 1, 0, None, None, 0, 0, 0) == -4
    assert G.eg3d_allreduce_claims(comm, 1, 0, None, C.c_void_p(ptr), n_cells, 0, 0) == -4
    assert G.eg3d_allreduce_claims(None, 1, 0, None, C.c_void_p(ptr), n_cells, 1, 0) == -1
    assert np.array_equal(ctx.fetch_dedup_claims(), before)
    # ---- the composition through the C ABI
    keep, n_kept = ctx.dedup_keep(local, base.value)
    assert n_kept == st["n_dedup_kept"]
    X_out, inlier, hist, n_inl, _ = ctx.gn_filter_device(local, keep, MSE)
    assert n_inl == st["n_gn_inliers"]
    thr = observation_threshold(hist, ctx.n_views, -1, count=n_inl)
    assert thr == st["threshold"]
    shard = ctx.compact_device(local, inlier, X_out, thr)
    out = D.DeviceEdgePoints()
    rp, ro = (C.c_uint64 * 1)(), (C.c_uint64 * 1)()
    assert G.eg3d_allgather_edgepoints(g, comm, 1, 0, None, C.byref(shard), C.byref(out), rp, ro) == 0
    assert rp[0] == want["n_points"] and ro[0] == want["n_obs"]
    assert same_cloud(ctx.fetch_device_points(out, 0, int(out.n_points)), want) is None
    # ---- and through the Python composition
    cloud, rc, thr2 = dedup_filter_then_gather(ctx, rg, None, 0, MSE)
    assert rc == 0 and thr2 == thr
    assert same_cloud(ctx.fetch_device_points(cloud, 0, int(cloud.n_points)), want) is None
    assert rg.exscan_points(n) == (0, n, 0)
    rg.close()
    ctx.close()


if __name__ == "__main__":
    main()
    print("RCCL-CLAIMS-OK")
