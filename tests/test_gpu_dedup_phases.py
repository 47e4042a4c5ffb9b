"""-m gpu: the 3 px dedup in phases (include/eg3d_dedup_phases.h). The C2 cloud's seeds cut in thirds, each part left in HBM by
a context of its own (as steps in flight are): claimed in any order on one context, or on two contexts whose maps are then
merged, and kept part by part, the parts give the mask of the whole cloud byte for byte (eg3d_host_filter_close_2d), and
the maps are eg3d_host_dedup_claim of the whole cloud cell for cell. The merge kernel alone on the map sizes where it can
go wrong, against np.minimum; the refusals; and, in a child process, a one-rank communicator through the whole C-ABI
composition. Everything is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dedup_cases as dc
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host
from edgegraph3d_amd.cloudnp import same_cloud
from dedup_gpu_cases import C2Cloud

pytestmark = pytest.mark.gpu
UNCLAIMED = 0xFFFFFFFF

_CACHE = {}


class C2Parts(C2Cloud):
    """The C2 cloud whole (self.dev, on self.ctx) and as the clouds of three seed ranges, each resident on a clone."""

    def __init__(self, rows):
        super().__init__(rows)
        n_seeds = int(self.s.seeds.contents.n_seeds)
        cuts = [0, n_seeds // 3, n_seeds // 2, n_seeds]   # as test_claims_across_calls
        self.clones, self.devs, self.bases = [], [], [0]
        for b, e in zip(cuts[:-1], cuts[1:]):
            cx = self.ctx.clone()
            self.clones.append(cx)
            r = cx.match_refpoints(self.s.seeds, b, e, device_only=True)
            dev = cx.last_device_output()
            assert dev.complete == 1 and int(dev.n_points) == r["n_points"] > 1000
            self.devs.append(dev)
            self.bases.append(self.bases[-1] + int(dev.n_points))
        assert self.bases[-1] == self.n
        for i, cx in enumerate(self.clones):   # the parts are the slices of the whole cloud
            assert same_cloud(cx.fetch_device_output(), dc.slice_cloud(self.cloud, self.bases[i], self.bases[i + 1])) is None

    def close(self):
        for cx in self.clones:
            cx.close()
        self.ctx.close()

    def keep_all(self, ctx):
        """The concatenated masks of the three parts against ctx's map, and the sum of the kept counts."""
        masks, total = [], 0
        for i, dev in enumerate(self.devs):
            k, n_kept = ctx.dedup_keep(dev, self.bases[i])
            masks.append(k.numpy(np.uint8)[:int(dev.n_points)])
            assert n_kept == int(masks[-1].sum()), i
            total += n_kept
        return np.concatenate(masks), total


def _drop_cache():
    import forms
    for rows, c in list(_CACHE.items()):
        with forms.product_form(rows):
            c.close()
    _CACHE.clear()


@pytest.fixture
def c2(eg3d_form):
    if eg3d_form not in _CACHE:
        _drop_cache()
        _CACHE[eg3d_form] = C2Parts(eg3d_form)
    return _CACHE[eg3d_form]


@pytest.fixture(scope="module", autouse=True)
def _close_cached_contexts():
    yield
    _drop_cache()


def _host_map(c2):
    return host.dedup_claim(c2.cloud, c2.V, c2.W, c2.H, host.dedup_empty_claims(c2.V, c2.W, c2.H), 0)


# ---- any order, one context ------------------------------------------------------------------------------------------------
def test_parts_claimed_in_reversed_order_on_one_context(c2):
    ctx = c2.ctx
    for i in (2, 1, 0):
        ctx.dedup_claim(c2.devs[i], c2.bases[i], reset=(i == 2))
    got, total = c2.keep_all(ctx)
    print("C2 in thirds, claimed 2-1-0: %d of %d kept" % (total, c2.n))
    assert np.array_equal(got, c2.dedup) and total == int(c2.dedup.sum())
    assert np.array_equal(ctx.fetch_dedup_claims(), _host_map(c2))
    # the combined call on the whole cloud afterwards is what it was
    k, n_kept = ctx.dedup_device(c2.dev)
    assert np.array_equal(k.numpy(np.uint8), c2.dedup) and n_kept == total
    # ... and the two forms mix: the combined call's claims serve a keep pass
    got, total = c2.keep_all(ctx)
    assert np.array_equal(got, c2.dedup)


# ---- two contexts and a merge ----------------------------------------------------------------------------------------------
def test_two_contexts_and_a_merge_in_each_direction(c2):
    A, B = c2.ctx, c2.clones[1]
    A.dedup_claim(c2.devs[0], c2.bases[0], reset=True)
    A.dedup_claim(c2.devs[2], c2.bases[2])
    B.dedup_claim(c2.devs[1], c2.bases[1], reset=True)
    a0, b0 = A.fetch_dedup_claims(), B.fetch_dedup_claims()
    assert not np.array_equal(a0, b0)
    low_a = A.dedup_merge_claims(B)
    a1 = A.fetch_dedup_claims()
    low_b = B.dedup_merge_claims(A)
    b1 = B.fetch_dedup_claims()
    print("merge: %d cells, %d lowered in A, %d in B; device time of the last merge %.3f ms" % (len(a0), low_a, low_b, B.dedup_phase_ms()))
    assert low_a == int((b0 < a0).sum()) > 0 and low_b == int((a1 < b0).sum()) > 0
    assert np.array_equal(a1, np.minimum(a0, b0)) and np.array_equal(a1, b1)     # all cells
    assert np.array_equal(a1, _host_map(c2))
    assert np.array_equal(A.fetch_dedup_claims(), a1)                             # (the second merge only read A)
    for ctx in (A, B):
        got, total = c2.keep_all(ctx)
        assert np.array_equal(got, c2.dedup) and total == int(c2.dedup.sum())
    # a map merged into itself, and merged again with what it already holds
    assert A.dedup_merge_claims(A) == 0 and B.dedup_merge_claims(A) == 0
    assert np.array_equal(A.fetch_dedup_claims(), a1) and np.array_equal(B.fetch_dedup_claims(), a1)
    # merging INTO a context that has no valid map makes one: fill, then min
    fresh = c2.clones[2]
    ptr, n_cells = A.dedup_claims()
    assert fresh.dedup_merge_claims(ptr, n_cells) == int((a1 != UNCLAIMED).sum())
    assert np.array_equal(fresh.fetch_dedup_claims(), a1)


# ---- shapes where the merge kernel can go wrong ----------------------------------------------------------------------------
# (V, cell columns, cell rows, word offsets of `other` from a 16-byte boundary). A lane takes one 16-byte word of four
# cells, a wavefront 64 words = 256 cells, a block 256 words = 1024 cells; K7B_MAX_BLOCKS = 2048 blocks cover 2 097 152
# cells, beyond which the grid goes round. The rigs have 3 or 4 views, so n_cells is a multiple of 3 or of 4.
MERGE_SHAPES = [
    (3, 1, 1, (1,)),            # 3 cells: no whole word, the tail alone
    (4, 1, 1, (1,)),            # 4: one word, no tail
    (3, 5, 3, (1,)),            # 45 = 11 words + 1
    (3, 17, 5, (1,)),           # 255: one wavefront of words less one cell (63 words + 3)
    (4, 8, 8, (1,)),            # 256: exactly one wavefront of words
    (3, 43, 2, (1,)),           # 258: one wavefront of words + 2 cells
    (4, 13, 5, (1,)),           # 260: one wavefront + one word
    (4, 17, 15, (1,)),          # 1020: one block less one word
    (3, 31, 11, (1,)),          # 1023: one block less one cell
    (4, 16, 16, (1,)),          # 1024: exactly one block
    (3, 19, 18, (1,)),          # 1026: one block + 2 cells
    (4, 257, 1, (1,)),          # 1028: one block + one word
    (3, 101, 37, (0, 1, 2, 3)),  # 11 211: eleven blocks and a tail of 3, every alignment of `other`
    (3, 1001, 800, (1,)),       # 2 402 400 > 2 097 152: the grid goes round
]


def _mix(rng, n):
    """A destination and an `other` of n cells: other is 0xFFFFFFFF, equal to, below, above the destination's entry, or 0."""
    dest = rng.integers(1, 2**32 - 1, n, dtype=np.uint64).astype(np.uint32)
    dest[rng.random(n) < 0.3] = UNCLAIMED
    dest[rng.random(n) < 0.05] = 0
    kind = rng.integers(0, 5, n)
    d64 = dest.astype(np.int64)
    below = np.maximum(d64 - rng.integers(1, 1000, n), 0)
    above = np.minimum(d64 + rng.integers(1, 1000, n), UNCLAIMED - 1)
    other = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [np.full(n, UNCLAIMED, np.int64), d64, below, above], 0)
    return dest, other.astype(np.uint32)


@pytest.fixture(scope="module")
def small_rigs():
    c3 = host.default_config(0)
    c3.n_views = 3
    return {3: host.Synth(c3), 4: host.Synth(0)}


def test_merge_kernel_on_the_map_sizes_where_it_can_go_wrong(eg3d_form, small_rigs):
    rng = np.random.default_rng(20261020)
    hip = api._hip()
    sizes = [V * w * h for V, w, h, _ in MERGE_SHAPES]
    assert min(sizes) < 4 and any(n % 4 for n in sizes) and max(sizes) > 2048 * 1024
    for V, w, h, offsets in MERGE_SHAPES:
        s = small_rigs[V]
        sc = dc.scene_with_size(s.scene, 3 * w - 1, max(1, 3 * h - 2))
        ctx = api.Context(C.byref(sc))
        try:
            assert ctx.n_views == V
            for word_off in offsets:
                ptr, n = ctx.dedup_claims()
                assert n == V * w * h
                dest, other = _mix(rng, n)
                assert hip.hipMemcpy(C.c_void_p(ptr), dest.ctypes.data, dest.nbytes, 1) == 0   # (entries only go down)
                lead = 4 + word_off
                buf = (0xA5000000 + np.arange(n + lead + 7, dtype=np.uint32)).astype(np.uint32)
                buf[lead:lead + n] = other
                dbuf = ctx.upload(buf)
                assert dbuf.ptr % 16 == 0 and (dbuf.ptr + 4 * lead) % 16 == 4 * word_off
                low = ctx.dedup_merge_claims(dbuf.ptr + 4 * lead, n)
                got = ctx.fetch_dedup_claims()
                assert np.array_equal(got, np.minimum(dest, other)), (V, w, h, word_off)
                assert low == int((other < dest).sum()), (V, w, h, word_off)
                # `other` and the words around it are as they were: the kernel writes the map alone, and nothing outside
                assert np.array_equal(dbuf.numpy(np.uint32), buf), (V, w, h, word_off)
        finally:
            ctx.close()


# ---- refusals (argument checks; nothing here reaches a kernel with bad data) ----------------------------------------------
def test_refusals(c2):
    L, ctx = api.lib(), c2.ctx
    n0 = int(c2.devs[0].n_points)
    keep = ctx.device_alloc(c2.n)
    # keep before any claim: a context that has claimed nothing holds no valid map
    fresh = ctx.clone()
    try:
        assert L.eg3d_dedup_keep(fresh._h, C.byref(c2.devs[0]), 0, keep.ptr, None) == -1
        assert b"claim" in L.eg3d_last_error()
        # ... the empty map asked for by name is one: nothing owns a cell, nothing is kept
        ptr, n_cells = fresh.dedup_claims()
        assert n_cells == c2.V * int(np.ceil(c2.W / 3)) * int(np.ceil(c2.H / 3))
        assert (fresh.fetch_dedup_claims() == UNCLAIMED).all()
        k, n_kept = fresh.dedup_keep(c2.devs[0], 0, keep)
        assert n_kept == 0 and not k.numpy(np.uint8)[:n0].any()
    finally:
        fresh.close()
    ctx.dedup_claim(c2.devs[0], 0, reset=True)
    before = ctx.fetch_dedup_claims()
    assert (before != UNCLAIMED).any()
    ptr, n_cells = ctx.dedup_claims()
    # merge with a wrong n_cells, a null or an odd address
    other = ctx.upload(np.zeros(n_cells + 4, np.uint32))
    for bad_n in (n_cells - 1, n_cells + 1, 0):
        assert L.eg3d_dedup_merge_claims(ctx._h, C.c_void_p(other.ptr), bad_n, None) == -1
        assert b"n_cells" in L.eg3d_last_error()
    assert L.eg3d_dedup_merge_claims(ctx._h, None, n_cells, None) == -1
    assert L.eg3d_dedup_merge_claims(ctx._h, C.c_void_p(other.ptr + 2), n_cells, None) == -1
    # index_base + n_points at the 2^32 - 1 limit
    assert L.eg3d_dedup_claim(ctx._h, C.byref(c2.devs[0]), 2**32 - 1 - n0, 0) == -1
    assert b"index_base" in L.eg3d_last_error()
    assert L.eg3d_dedup_keep(ctx._h, C.byref(c2.devs[0]), 2**32 - 1 - n0, keep.ptr, None) == -1
    assert b"index_base" in L.eg3d_last_error()
    # null arguments, a view that is not complete
    assert L.eg3d_dedup_claim(ctx._h, None, 0, 0) == -1 and L.eg3d_dedup_claim(None, C.byref(c2.devs[0]), 0, 0) == -1
    assert L.eg3d_dedup_keep(ctx._h, C.byref(c2.devs[0]), 0, None, None) == -1
    assert L.eg3d_dedup_claims(ctx._h, None, None) == -1
    part = c2.view(c2.n)
    part.complete = 0
    assert L.eg3d_dedup_claim(ctx._h, C.byref(part), 0, 0) == -1
    # a cloud whose offsets do not ascend (one list in the middle; the last list beyond n_obs), with and without a reset
    for where, value in ((c2.n // 3, None), (c2.n - 1, int(c2.cloud["n_obs"]) + 1)):
        off = c2.cloud["obs_off"][:-1].copy()
        off[where] = off[where + 1] + 5 if value is None else value
        bad = c2.view(c2.n)
        od = ctx.upload(off)
        bad.obs_off = od.ptr
        for reset in (0, 1):
            assert L.eg3d_dedup_claim(ctx._h, C.byref(bad), 0, reset) == -1
            assert b"obs_off" in L.eg3d_last_error()
    # none of it touched the map: cell for cell what it was, and the earlier part's claims still give the right mask
    assert np.array_equal(ctx.fetch_dedup_claims(), before)
    k, n_kept = ctx.dedup_keep(c2.devs[0], 0, keep)
    assert np.array_equal(k.numpy(np.uint8)[:n0], c2.dedup[:n0]) and n_kept == int(c2.dedup[:n0].sum())
    # the largest index_base that fits
    top = 2**32 - 2 - c2.n
    ctx.dedup_claim(c2.dev, top, reset=True)
    k, n_kept = ctx.dedup_keep(c2.dev, top, keep)
    assert np.array_equal(k.numpy(np.uint8), c2.dedup) and int(ctx.fetch_dedup_claims().min()) >= top


# ---- one rank through RCCL, in a process of its own ------------------------------------------------------------------------
def test_single_rank_through_rccl(eg3d_form):
    """tests/rccl_claims_single_rank_check.py: librccl must not share a process with the HIP runtime of the torch wheel."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "rccl_claims_single_rank_check.py")], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "RCCL-CLAIMS-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
