"""The matches manager of a sharded run over ranks (CPU, gloo): distributed.replay_merge_ranks on the host statements. The
oracle's cloud of the C2 window is cut at chain boundaries into one shard per rank (world 4: one rank's shard is empty); every
rank replays its shard alone (host.replay_matches), the graphs are gathered and folded in rank order into a host.ReplayState,
and every rank must end with exactly the graph one process builds from the whole cloud — the oracle's replay_matches — field
for field and bit for bit. At most 4 CPU processes; none opens a GPU."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import replay_gpu_cases as rc
from edgegraph3d_amd import host
from edgegraph3d_amd.distributed import replay_merge_ranks
from test_replay_accumulate import chain_starts, slice_cloud

CFG, WINDOW = 2, (1550, 1800)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, shard, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = host.Synth(CFG)
    st = host.ReplayState(s.scene)
    try:
        mine = host.replay_matches(s.scene, shard)
        g = replay_merge_ranks(st, dist, mine, shard["n_points"])
        q.put((rank, g, st.n_points, [mine["n_nodes"], mine["n_polylines"], int(mine["iv_off"][-1])]))
    finally:
        st.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world,bounds", [(2, (0, 1 / 3, 1)), (4, (0, 0.2, 0.5, 0.5, 1))], ids=["2 ranks", "4 ranks, one empty"])
def test_every_rank_ends_with_the_single_process_graph(world, bounds):
    from oracle import binding as ob
    s = host.Synth(CFG)
    o = ob.Oracle(s.scene)
    whole = o.match(s.seeds, WINDOW[0], WINDOW[1], 16)
    want = o.replay_matches(whole)
    n = int(whole["n_points"])
    starts = np.array([0] + chain_starts(whole) + [n])
    cuts = [int(starts[np.searchsorted(starts, int(n * b))]) for b in bounds]      # the chain boundary at or after the fraction
    shards = [slice_cloud(whole, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    assert len(shards) == world and shards[0]["n_points"] > 2 and sum(sh["n_points"] for sh in shards) == n
    assert (world == 2) or any(sh["n_points"] == 0 for sh in shards)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, shards[r], q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {r: rest for r, *rest in (q.get(timeout=240) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    separate = np.sum([got[r][2] for r in range(world)], axis=0)
    # (the shards' graphs hold more than the whole: concatenating them would not pass)
    assert (separate > [want["n_nodes"], want["n_polylines"], int(want["iv_off"][-1])]).all(), separate
    for r in range(world):
        g, points, _ = got[r]
        assert points == n, (r, points)
        assert rc.same_graph(g, want) is None, (r, rc.same_graph(g, want))
