#!/usr/bin/env python3
"""Two-rank check of include/eg3d_rccl_claims.h for a node with >= 2 GPUs, beside tests/rccl_two_rank_check.py and in its
pattern (no torch; the unique id travels through a file). NOT part of the suite and not yet run anywhere: no machine with
more than one GPU has been available. tests/test_dedup_phases_gloo.py runs the same composition on CPU ranks and
tests/rccl_claims_single_rank_check.py the same calls on a communicator of one rank.

    python tests/rccl_claims_two_rank_check.py            # ranks 0 and 1 (GPUs 0 and 1), prints RCCL-CLAIMS-2RANK-OK
    python tests/rccl_claims_two_rank_check.py --world 4

Every rank matches its balanced share of the small synthetic scene's seeds and runs exscan -> claim -> all-reduce (whole,
and in 4 KiB pieces) -> keep -> filter -> threshold -> compact -> gather; every rank must end with what
eg3d_dedup_resident(with_filter = 1) gives on the cloud of all seeds (computed on every rank by itself). Then the
agreement round: the last rank passes local_ok = 0, every rank gets -4; the last rank passes one cell less, every rank -1.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MSE = 2.25


def worker(rank, world, idfile):
    from edgegraph3d_amd import _cdefs as D
    from edgegraph3d_amd import api, host
    from edgegraph3d_amd.cloudnp import same_cloud
    from edgegraph3d_amd.distributed import gather_lib, shard_ranges_balanced
    G = gather_lib()
    uid = (C.c_ubyte * 128)()
    if rank == 0:
        assert G.eg3d_comm_unique_id(uid) == 0
        with open(idfile + ".tmp", "wb") as f:
            f.write(bytes(uid))
        os.rename(idfile + ".tmp", idfile)
    else:
        for _ in range(600):
            if os.path.exists(idfile):
                break
            time.sleep(0.1)
        C.memmove(uid, open(idfile, "rb").read(), 128)
    comm = C.c_void_p()
    assert G.eg3d_comm_init(uid, world, rank, rank, C.byref(comm)) == 0
    g = G.eg3d_gather_create(rank)
    s = host.Synth(1)
    ctx = api.Context(s.scene, rank)
    ctx.upload_seeds(s.seeds)
    ctx.match_resident(0, s.n_seeds, device_only=True)
    want, _, st = ctx.dedup_resident(with_filter=True, gn_max_mse=MSE)
    b, e = shard_ranges_balanced(s.seeds_np()[0], 0, s.n_seeds, world)[rank]
    for chunk in (0, 4096):
        ctx.match_resident(b, e, device_only=True)
        local = ctx.last_device_output()
        base, total = C.c_uint64(0), C.c_uint64(0)
        assert G.eg3d_exscan_points(comm, world, rank, None, int(local.n_points), C.byref(base), C.byref(total)) == 0
        assert total.value == st["n_points_in"]
        ctx.dedup_claim(local, base.value, reset=True)
        ptr, n_cells = ctx.dedup_claims()
        assert G.eg3d_allreduce_claims(comm, world, rank, None, C.c_void_p(ptr), n_cells, 1, chunk) == 0
        keep, _ = ctx.dedup_keep(local, base.value)
        X_out, inlier, hist, n_inl, _ = ctx.gn_filter_device(local, keep, MSE)
        # (no torch here to sum the histograms: the threshold of the whole cloud, which the summed histogram gives —
        # tests/test_filter_threshold_gloo.py — is taken from the single-process call)
        shard = ctx.compact_device(local, inlier, X_out, st["threshold"])
        out = D.DeviceEdgePoints()
        assert G.eg3d_allgather_edgepoints(g, comm, world, rank, None, C.byref(shard), C.byref(out), None, None) == 0
        assert same_cloud(ctx.fetch_device_points(out, 0, int(out.n_points)), want) is None, (rank, chunk)
        print("rank %d: pieces of %d B ok (%d of %d points survive)" % (rank, chunk, int(out.n_points), total.value), flush=True)
    last = rank == world - 1
    assert G.eg3d_allreduce_claims(comm, world, rank, None, C.c_void_p(ptr), n_cells, 0 if last else 1, 0) == -4
    assert G.eg3d_allreduce_claims(comm, world, rank, None, C.c_void_p(ptr), n_cells - (1 if last else 0), 1, 0) == -1
    print("rank %d: both refusals of the agreement round reached every rank" % rank, flush=True)
    G.eg3d_gather_destroy(g)
    G.eg3d_comm_destroy(comm)
    ctx.close()


def main():
    if "--rank" in sys.argv:
        i = sys.argv.index("--rank")
        worker(int(sys.argv[i + 1]), int(sys.argv[i + 2]), sys.argv[i + 3])
        return
    world = int(sys.argv[sys.argv.index("--world") + 1]) if "--world" in sys.argv else 2
    with tempfile.TemporaryDirectory() as d:
        idfile = os.path.join(d, "nccl_id")
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(r), str(world), idfile])
                 for r in range(world)]
        rcs = [p.wait(timeout=600) for p in procs]
    if any(rcs):
        raise SystemExit("rccl claims two-rank check failed: %s" % rcs)
    print("RCCL-CLAIMS-2RANK-OK")


if __name__ == "__main__":
    main()
