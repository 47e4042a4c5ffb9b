"""The observation threshold of a cloud that is spread over ranks (CPU, gloo): every rank contributes the histogram of
ITS shard's list lengths, global_observation_threshold all-reduces them and applies the rule of
eg3d_host_observation_filter; the result must be what that host function returns on the concatenation of the shards
(with the caller's SfM points in front, as the reference keeps them, when base_hist is given). One rank holds an
empty shard. The cases span medians small enough for the floor of 3 and large enough for median / 2 - 1."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import host
from edgegraph3d_amd.distributed import global_observation_threshold, observation_threshold

N_VIEWS = 24
CASES = [(3, 9), (9, 24), (2, 30)]  # list lengths drawn from [lo, hi] (30 > N_VIEWS: lists that sit in no bin)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard(case, rank, world, empty_rank):
    lo, hi = CASES[case]
    rng = np.random.default_rng(1000 * case + rank)
    n = 0 if rank == empty_rank else 400 + 150 * rank
    return rng.integers(lo, hi + 1, n).astype(np.int64)


def _sfm(case):
    return np.random.default_rng(77 + case).integers(2, 7, 900).astype(np.int64)


def _hist(k):
    return np.bincount(k[k <= N_VIEWS], minlength=N_VIEWS + 1).astype(np.int64)


def _host_threshold(k_all, first_edgepoint, forced):
    off = np.concatenate([[0], np.cumsum(k_all)]).astype(np.uint32)
    inl = np.ones(len(k_all), np.uint8)
    return host.lib().eg3d_host_observation_filter(N_VIEWS, D.np_ptr(off, C.c_uint32), len(k_all), first_edgepoint, forced,
                                                   D.np_ptr(inl, C.c_uint8))


def _worker(rank, world, port, empty_rank, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for case in range(len(CASES)):
        k = _shard(case, rank, world, empty_rank)
        for with_base in (False, True):
            for forced in (-1, 4):
                out[(case, with_base, forced)] = global_observation_threshold(
                    dist, _hist(k), N_VIEWS, forced, _hist(_sfm(case)) if with_base else None, local_count=len(k))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world,empty_rank", [(2, 1), (4, 2)], ids=["2 ranks", "4 ranks"])
def test_global_threshold_equals_the_host_filter_on_the_concatenation(world, empty_rank):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, empty_rank, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    seen = set()
    for case in range(len(CASES)):
        k_all = np.concatenate([_shard(case, r, world, empty_rank) for r in range(world)])
        for with_base in (False, True):
            sfm = _sfm(case) if with_base else np.zeros(0, np.int64)
            for forced in (-1, 4):
                want = _host_threshold(np.concatenate([sfm, k_all]), len(sfm), forced)
                for r in range(world):
                    assert got[r][(case, with_base, forced)] == want, (case, with_base, forced, r)
                if forced < 0:
                    seen.add(want)
    assert 3 in seen and max(seen) > 3, seen   # the floor and the median rule both decided a case


def test_threshold_rule_on_one_process():
    """The same rule without a process group (dist = None), against the host function, over many shapes."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        lo = int(rng.integers(0, 12))
        k = rng.integers(lo, lo + int(rng.integers(1, 20)), int(rng.integers(0, 300))).astype(np.int64)
        forced = int(rng.choice([-1, -1, 0, 4]))
        want = _host_threshold(k, 0, forced)
        assert global_observation_threshold(None, _hist(k), N_VIEWS, forced, local_count=len(k)) == want
        assert observation_threshold(_hist(k), N_VIEWS, forced, count=len(k)) == want
