"""The reference-exact end of a sharded step over ranks (CPU, gloo): distributed.dedup_filter_then_gather on HostShard
(the host statements of the phased dedup, the CPU oracle's Gauss-Newton verdict) and HostCloudGather. The oracle's cloud of
synthetic config 1 is cut BETWEEN POINTS into one shard per rank (world 4: one rank's shard is empty); every rank must end
with exactly what one process computes on the whole cloud in the reference's order — dedup, filter, threshold, compact —
all seven arrays bit for bit. Then the two ways the claim exchange can refuse: ranks that disagree on the number of cells,
and a rank whose claim failed; every rank gets the same code and none blocks. At most 4 CPU processes; none opens a GPU."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import dedup_cases as dc
from edgegraph3d_amd import host
from edgegraph3d_amd.cloudnp import np_compact, same_cloud
from edgegraph3d_amd.distributed import HostCloudGather, HostShard, dedup_filter_then_gather
from dedup_gpu_cases import host_threshold

CFG, MSE = 1, 2.25
FORCED = (-1, 4)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oracle_filter(o, cloud, mse, legacy=False):
    return o.gn_filter(cloud["X"], cloud["obs_off"].astype(np.uint32), cloud["obs_view"], cloud["obs_xy"], mse,
                       legacy_abs=legacy, nthreads=2)


def _worker(rank, world, port, shard, q):
    from oracle import binding as ob
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = host.Synth(CFG)
    o = ob.Oracle(s.scene)
    sc = s.scene.contents
    V, W, H = int(sc.n_views), int(sc.width), int(sc.height)
    gather = HostCloudGather(dist, world, rank)
    gn = lambda c, mse, legacy: _oracle_filter(o, c, mse, legacy)   # noqa: E731
    out = {}
    for forced in FORCED:
        stage = HostShard(shard, V, W, H, gn)
        cloud, rc, thr = dedup_filter_then_gather(stage, gather, dist, 0, MSE, False, forced)
        out[forced] = (cloud, rc, thr)
    # ranks that do not describe the same rig: the last rank's map has another number of cells
    odd = HostShard(shard, V, W + (3 if rank == world - 1 else 0), H, gn)
    out["cells"] = dedup_filter_then_gather(odd, gather, dist, 0, MSE)
    # a rank whose claim fails (offsets that do not ascend on rank 0; an empty shard cannot fail: its rank stays sound)
    broken = dict(shard)
    if rank == 0:
        broken["obs_off"] = shard["obs_off"].copy()
        broken["obs_off"][1] = broken["obs_off"][2] + 5
    out["claim"] = dedup_filter_then_gather(HostShard(broken, V, W, H, gn), gather, dist, 0, MSE)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world,bounds", [(2, (0, 1 / 3, 1)), (4, (0, 0.2, 0.5, 0.5, 1))], ids=["2 ranks", "4 ranks, one empty"])
def test_every_rank_ends_with_the_single_process_result(world, bounds):
    from oracle import binding as ob
    s = host.Synth(CFG)
    o = ob.Oracle(s.scene)
    whole = o.match(s.seeds, 0, int(s.seeds.contents.n_seeds), 16)
    sc = s.scene.contents
    V, W, H = int(sc.n_views), int(sc.width), int(sc.height)
    n = int(whole["n_points"])
    cuts = [min(n, int(n * b) + (1 if 0 < b < 1 else 0)) for b in bounds]
    shards = [dc.slice_cloud(whole, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    assert len(shards) == world and shards[0]["n_points"] > 2
    assert (world == 2) or any(sh["n_points"] == 0 for sh in shards)
    # one process, the reference's order
    dedup = dc.host_mask(whole, V, W, H)
    small = np_compact(whole, dedup)
    Xs, inls = _oracle_filter(o, small, MSE)
    want = {}
    for forced in FORCED:
        thr, surv = host_threshold(V, np.diff(small["obs_off"].astype(np.int64)), inls, forced)
        want[forced] = (thr, np_compact(small, surv, Xs))
        assert 0 < want[forced][1]["n_points"] < small["n_points"] < n
    # (a shard deduplicated on its own would keep more: the exchange of the claims is what this test is about)
    assert dc.host_mask(shards[-1], V, W, H).sum() > dedup[cuts[-2]:].sum()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, shards[r], q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(world):
        for forced in FORCED:
            cloud, rc, thr = got[r][forced]
            assert rc == 0 and thr == want[forced][0], (r, forced, rc, thr)
            assert same_cloud(cloud, want[forced][1]) is None, (r, forced)
        assert got[r]["cells"] == (None, -1, None), (r, got[r]["cells"])
        assert got[r]["claim"] == (None, -4, None), (r, got[r]["claim"])
