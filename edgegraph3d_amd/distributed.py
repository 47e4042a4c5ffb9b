"""Multi-GPU plumbing of the path: seed sharding and the all-gather of the edge-point cloud.

One process per GPU (torch.distributed for rendezvous; RCCL over xGMI for the exchange; "gloo" on CPU
for tests). Seeds are independent units, so rank r owns the contiguous range
shard_ranges_balanced(...)[r] (balanced by the sum of track lengths; shard_range = by count)
and the concatenation of the per-rank outputs in rank order IS the single-process output. The
only exchange step is the variable-length all-gather of the cloud (include/eg3d_rccl.h): counts first
(24 B/rank), then the seven arrays of every rank's cloud
    X(12 B/pt) | obs_off(8) | key(16) | obs_view(4/obs) | obs_pl(4) | obs_seg(4) | obs_xy(8)
travel straight to their final position in every receiver's result arrays (no packing or padding), and
the observation offsets of ranks > 0 are rebased. RcclCloudGather = the C-ABI entry point on GPUs;
HostCloudGather = the same plan on host arrays around any torch.distributed backend.
"""
import torch

FIELDS = (("X", 12, True), ("obs_off", 8, True), ("key", 16, True), ("obs_view", 4, False), ("obs_pl", 4, False),
          ("obs_seg", 4, False), ("obs_xy", 8, False))  # name, bytes per element, per point (else per observation)


def shard_range(n_seeds, world):
    """Contiguous, count-balanced seed ranges [(begin, end)] per rank."""
    base, rem = divmod(n_seeds, world)
    out, b = [], 0
    for r in range(world):
        e = b + base + (1 if r < rem else 0)
        out.append((b, e))
        b = e
    return out


def shard_ranges_balanced(trk_off, begin, end, world):
    """Contiguous seed ranges of [begin, end) per rank, balanced by the sum of the track lengths k
    (the loop being split, plg_matching_from_refpoints.cpp:83-104, costs ~k candidate searches and
    ~k start views per seed) instead of by seed count. trk_off = the seeds' CSR offsets, so the
    weight of a range is one subtraction. Every rank computes the same split from the same array."""
    import numpy as np
    off = np.asarray(trk_off, dtype=np.int64)
    lo, hi = int(off[begin]), int(off[end])
    cuts = [begin]
    for r in range(1, world):
        target = lo + (hi - lo) * r // world
        c = int(np.searchsorted(off[begin:end + 1], target, side="left")) + begin
        cuts.append(min(max(c, cuts[-1]), end))
    cuts.append(end)
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


class StepPlan:
    """Which seeds a rank takes in step i of the multi-GPU workload — the ONE statement of it: bench.py's Leg uses this
    object, and tests/test_multirank_gloo.py runs the same object on CPU ranks. A step = one batch of `batch` seeds
    (bench.py --gpus N: 4096 x N), split over the ranks into contiguous ranges balanced by the sum of track lengths;
    rank order = seed order, so the concatenation of the ranks' clouds is the batch's cloud."""

    def __init__(self, trk_off, n_total, batch, world, rank):
        self.trk_off, self.n_total, self.world, self.rank = trk_off, int(n_total), int(world), int(rank)
        self.batch = max(1, min(int(batch), self.n_total)) if self.n_total else 1
        self.n_batches = max(1, self.n_total // self.batch)   # whole batches: the timed steps cycle through them

    def batch_bounds(self, i, cyclic=True):
        b0 = ((i % self.n_batches) if cyclic else i) * self.batch
        return b0, min(b0 + self.batch, self.n_total)

    def step_range(self, i):
        """Timed step i: batch i (cyclic over the WHOLE batches), this rank's share."""
        b0, b1 = self.batch_bounds(i, True)
        return shard_ranges_balanced(self.trk_off, b0, b1, self.world)[self.rank]

    def pass_range(self, i):
        """Step i of ONE pass over all seeds: ceil(n / batch) steps, the last one partial."""
        b0, b1 = self.batch_bounds(i, False)
        return shard_ranges_balanced(self.trk_off, b0, b1, self.world)[self.rank]

    def n_pass_steps(self):
        return (self.n_total + self.batch - 1) // self.batch


class SetsPlan:
    """Which ITEMS of resident polyline sets a rank takes (include/eg3d_sets_device.h), in the shape of StepPlan: pure
    arithmetic on the per-item sample counts that Context.polyline_item_samples returns. The items [0, n) are split into
    `world` contiguous ranges balanced by the samples; rank order = item order, and sample_base(rank) — the samples of the
    ranks before — is what the rank passes to Context.match_polyline_items, so that the concatenation of the ranks' clouds
    is the cloud of one call over all items. Rank k's range ends at the first item boundary at which the samples so far
    reach k + 1 shares of the total, so no share exceeds the ideal (total / world) by as much as its largest item. Items
    without samples travel with the range they fall into; with no samples at all the items are split evenly."""

    def __init__(self, counts, world, rank=0):
        import numpy as np
        self.world, self.rank = int(world), int(rank)
        if self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError("SetsPlan: need world >= 1 and 0 <= rank < world")
        c = np.asarray(counts, np.int64).reshape(-1)
        if (c < 0).any():
            raise ValueError("SetsPlan: a sample count is negative")
        self.n_items = len(c)
        self.prefix = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
        self.total = int(self.prefix[-1])
        k = np.arange(1, self.world, dtype=np.int64)
        if self.total:
            # first boundary whose prefix reaches k shares (k * total / world, compared exactly in integers)
            inner = np.searchsorted(self.prefix * self.world, k * self.total, side="left")
        else:
            inner = (k * self.n_items) // self.world
        self.cuts = np.concatenate([[0], inner, [self.n_items]]).astype(np.int64)

    def item_range(self, rank=None):
        r = self.rank if rank is None else int(rank)
        return int(self.cuts[r]), int(self.cuts[r + 1])

    def sample_base(self, rank=None):
        return int(self.prefix[self.item_range(rank)[0]])

    def n_samples(self, rank=None):
        b, e = self.item_range(rank)
        return int(self.prefix[e] - self.prefix[b])

    def ranges(self):
        """[(item_begin, item_end, sample_base)] of every rank, in rank order."""
        return [self.item_range(r) + (self.sample_base(r),) for r in range(self.world)]


_GATHER_LIB = None


def gather_lib():
    """libeg3d_rccl.so with include/eg3d_rccl.h declared on it. Loaded on first use, never on import: it brings librccl
    into the process, which only a caller of the exchange wants."""
    global _GATHER_LIB
    if _GATHER_LIB is None:
        import ctypes as C
        import os
        from ._cabi import bind_library
        _GATHER_LIB = bind_library(C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libeg3d_rccl.so")), "rccl")
    return _GATHER_LIB


class RcclCloudGather:
    """The C-ABI exchange step (include/eg3d_rccl.h: eg3d_allgather_edgepoints in libeg3d_rccl.so) on an
    RCCL communicator created by the same library (eg3d_comm_init: hipSetDevice + ncclCommInitRank); the
    unique id travels through the caller's existing torch.distributed group (any backend)."""

    def __init__(self, dist, world, rank, device_index, stream_ptr=None):
        import ctypes as C
        import os
        import torch as _t
        from . import _cdefs as D
        self.C, self.D = C, D
        self.world, self.rank = world, rank
        self.g, self.comm = None, None
        self.G = gather_lib()
        uid = (C.c_ubyte * 128)()
        if rank == 0:
            rc = self.G.eg3d_comm_unique_id(uid)
            if rc != 0:
                raise RuntimeError("eg3d_comm_unique_id failed (%d)" % rc)
        if world > 1:
            dev = _t.device("cuda", device_index) if dist.get_backend() == "nccl" else _t.device("cpu")
            t = _t.tensor(list(bytes(uid)), dtype=_t.uint8, device=dev)
            dist.broadcast(t, src=0)
            raw = bytes(t.cpu().numpy().tobytes())
            C.memmove(uid, raw, 128)
        self.comm = C.c_void_p()
        rc = self.G.eg3d_comm_init(uid, world, rank, device_index, C.byref(self.comm))
        if rc != 0:
            raise RuntimeError("eg3d_comm_init (hipSetDevice + ncclCommInitRank) failed (%d) on rank %d" % (rc, rank))
        # pre-flight, part 1: what RCCL itself reports about the communicator must be what the launcher started
        n_, r_, d_ = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        rc = self.G.eg3d_comm_query(self.comm, C.byref(n_), C.byref(r_), C.byref(d_))
        self.comm_info = {"ncclCommCount": n_.value, "ncclCommUserRank": r_.value, "ncclCommCuDevice": d_.value}
        import sys as _sys
        print("RCCL-PREFLIGHT rank %d/%d: ncclCommCount=%d ncclCommUserRank=%d device=%d (rc %d)"
              % (rank, world, n_.value, r_.value, d_.value, rc), file=_sys.stderr, flush=True)
        if rc != 0 or n_.value != world or r_.value != rank or d_.value != device_index:
            self.close()
            raise RuntimeError("RCCL pre-flight: the communicator reports %s, expected %d ranks / rank %d / device %d"
                               % (self.comm_info, world, rank, device_index))
        self.g = self.G.eg3d_gather_create(device_index)
        if not self.g:
            self.close()  # do not leak the communicator
            raise RuntimeError("eg3d_gather_create failed")
        self.stream = C.c_void_p(stream_ptr) if stream_ptr else None
        self.rank_points = (C.c_uint64 * world)()
        self.rank_obs = (C.c_uint64 * world)()
        self.mode = "bcast" if os.environ.get("EG3D_GATHER_MODE", "")[:1] in ("b", "1") else "sendrecv"
        self.selftest = None
        if world > 1 and dist.get_backend() == "nccl":
            self._choose_mode(dist, device_index)

    # ---- pre-flight check of the exchange (multi-rank only) -------------------------------------------------
    def _selftest_once(self, device_index):
        """A tiny hand-made cloud per rank (rank r: 2 + r points; odd ranks' points carry two observations each, even
        ranks' none — zero-size arrays on some pairs) through eg3d_allgather_edgepoints; True when this rank holds exactly
        the concatenation every rank can predict."""
        import numpy as np
        import torch as _t
        C, D = self.C, self.D
        dev = _t.device("cuda", device_index)

        def cloud(r):
            n = 2 + r
            k = 2 if r % 2 else 0
            X = (np.arange(3 * n, dtype=np.float32) + 1000.0 * r).reshape(n, 3)
            key = (np.arange(4 * n, dtype=np.int64) + 7 * r).astype(np.uint32).reshape(n, 4)
            off = (np.arange(n + 1, dtype=np.uint64) * k)
            m = n * k
            view = (np.arange(m, dtype=np.int32) + r)
            pl = (np.arange(m, dtype=np.int64) * 3 + r).astype(np.uint32)
            seg = (np.arange(m, dtype=np.int64) * 5 + r).astype(np.uint32)
            xy = (np.arange(2 * m, dtype=np.float32) * 0.5 + r).reshape(m, 2)
            return X, off, key, view, pl, seg, xy

        mine = cloud(self.rank)
        keep = [_t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) if a.size else
                _t.zeros(16, dtype=_t.uint8, device=dev) for a in mine]
        loc = D.DeviceEdgePoints()
        loc.n_points, loc.n_obs, loc.complete = len(mine[0]), len(mine[3]), 1
        loc.X, loc.obs_off, loc.key, loc.obs_view, loc.obs_pl, loc.obs_seg, loc.obs_xy = [t.data_ptr() for t in keep]
        out = D.DeviceEdgePoints()
        _t.cuda.synchronize(dev)
        rc = self.G.eg3d_allgather_edgepoints(self.g, self.comm, self.world, self.rank, self.stream, C.byref(loc), C.byref(out),
                                              self.rank_points, self.rank_obs)
        if rc != 0:
            return rc, False
        parts = [cloud(r) for r in range(self.world)]
        want_X = np.concatenate([p[0] for p in parts])
        want_key = np.concatenate([p[2] for p in parts])
        obase, want_off = 0, [np.zeros(1, np.uint64)]
        for p in parts:
            want_off.append(p[1][1:] + np.uint64(obase))
            obase += len(p[3])
        want_off = np.concatenate(want_off)
        want = [want_X, want_off, want_key] + [np.concatenate([p[i] for p in parts]) for i in (3, 4, 5, 6)]
        if int(out.n_points) != len(want_X) or int(out.n_obs) != obase:
            return 0, False
        try:
            hip = C.CDLL("libamdhip64.so.7")
        except OSError:
            hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        ptrs = [out.X, out.obs_off, out.key, out.obs_view, out.obs_pl, out.obs_seg, out.obs_xy]
        for w, ptr in zip(want, ptrs):
            w = np.ascontiguousarray(w)
            got = np.empty_like(w)
            if w.nbytes and hip.hipMemcpy(got.ctypes.data, C.c_void_p(ptr), w.nbytes, 2) != 0:
                return 0, False
            if not np.array_equal(got.view(np.uint8), w.view(np.uint8)):
                return 0, False
        return 0, True

    def _choose_mode(self, dist, device_index):
        """The grouped send/recv exchange is the default; if the pre-flight cloud does not come out right on EVERY rank
        (an RCCL build on which it misbehaves), all ranks switch to the broadcast fallback together and test that."""
        import torch as _t
        dev = _t.device("cuda", device_index)
        tried = []
        for mode in ([self.mode] if self.mode == "bcast" else ["sendrecv", "bcast"]):
            self.G.eg3d_gather_set_mode(self.g, 1 if mode == "bcast" else 0)
            rc, ok = self._selftest_once(device_index)
            # [0] = ranks whose data came out wrong, [1] = ranks whose call FAILED (rc != 0: with EG3D_GATHER_ERR_FATAL the
            # library has already aborted the communicator on that rank — it must not be used again, by anyone)
            t = _t.tensor([0 if ok or rc != 0 else 1, 1 if rc != 0 else 0], dtype=_t.int32, device=dev)
            dist.all_reduce(t)
            bad_data, failed = int(t[0].item()), int(t[1].item())
            tried.append((mode, bad_data == 0 and failed == 0))
            if failed:
                # a failed call is not a reason to try the other mode on the same communicator: give it up on every rank
                self.selftest = tried
                if rc == -6:
                    self.abandon_comm()
                self.close()
                raise RuntimeError("eg3d_allgather_edgepoints failed (rc %d on this rank, %d rank(s) failed) in its pre-flight "
                                   "check, mode %s: the communicator is abandoned" % (rc, failed, mode))
            if tried[-1][1]:
                self.mode = mode
                self.selftest = tried
                return
        self.selftest = tried
        self.close()
        raise RuntimeError("eg3d_allgather_edgepoints failed its pre-flight check in every exchange mode: %s" % tried)

    def allgather(self, local_dev):
        """local_dev = Context.last_device_output(), or None when this rank has no usable result (its match
        failed): it still takes part, and the status word makes EVERY rank return EG3D_GATHER_ERR_INCOMPLETE (-4)
        instead of leaving the others inside the collective. Returns (DeviceEdgePoints of the whole cloud, rc);
        every rank gets the same rc (see include/eg3d_rccl.h)."""
        C = self.C
        out = self.D.DeviceEdgePoints()
        rc = self.G.eg3d_allgather_edgepoints(self.g, self.comm, self.world, self.rank, self.stream,
                                              C.byref(local_dev) if local_dev is not None else None, C.byref(out),
                                              self.rank_points, self.rank_obs)
        if rc == -6:
            self.abandon_comm()
        return out, rc

    # ---- the exchanges of the dedup in phases (include/eg3d_rccl_claims.h) ----
    def exscan_points(self, n_points):
        """eg3d_exscan_points: (points of the lower ranks, points of all ranks, rc); the same rc on every rank."""
        C = self.C
        base, total = C.c_uint64(0), C.c_uint64(0)
        rc = self.G.eg3d_exscan_points(self.comm, self.world, self.rank, self.stream, int(n_points), C.byref(base), C.byref(total))
        if rc == -6:
            self.abandon_comm()
        return int(base.value), int(total.value), rc

    def allreduce_claims(self, ctx, chunk_bytes=0):
        """eg3d_allreduce_claims on the claim map of `ctx` (a Context), in place: afterwards every rank's map holds the
        claims of all ranks. ctx = None: this rank has no usable map (its claim failed); it still takes part, and every
        rank returns EG3D_GATHER_ERR_INCOMPLETE (-4) before any payload moves. Returns rc, the same on every rank."""
        ptr, n_cells = ctx.dedup_claims() if ctx is not None else (None, 0)
        rc = self.G.eg3d_allreduce_claims(self.comm, self.world, self.rank, self.stream, ptr, n_cells, 1 if ctx is not None else 0,
                                          int(chunk_bytes))
        if rc == -6:
            self.abandon_comm()
        return rc

    def close(self):
        if getattr(self, "g", None):
            self.G.eg3d_gather_destroy(self.g)
            self.g = None
        if getattr(self, "comm", None):
            self.G.eg3d_comm_destroy(self.comm)
            self.comm = self.C.c_void_p()

    def abandon_comm(self):
        """After EG3D_GATHER_ERR_FATAL (-6) the library has aborted the communicator: forget it."""
        self.comm = self.C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostCloudGather:
    """The exchange on HOST arrays over any torch.distributed backend (gloo on CPU): the transport is one
    broadcast per (rank, array) of the raw bytes; the plan (bases, totals, status) and the placement + rebasing
    of every rank's cloud are the C functions eg3d_host_gather_plan / eg3d_host_gather_place of libeg3d_host.so —
    the same arithmetic eg3d_allgather_edgepoints applies to device buffers."""

    def __init__(self, dist, world, rank):
        from . import host as _host
        self.dist, self.world, self.rank = dist, world, rank
        self.H = _host.lib()

    def allgather(self, local):
        """local = a cloud dict as the C ABI returns it (obs_off with its sentinel), or None for "this rank has
        no usable result". Returns (whole cloud dict or None, rc), the same rc on every rank."""
        import ctypes as C
        import numpy as np
        from . import _cdefs as D
        dist, world, rank = self.dist, self.world, self.rank
        mine = [int(local["n_points"]), int(local["n_obs"]), 0] if local is not None else [0, 0, 1]
        allc = torch.empty(3 * world, dtype=torch.int64)
        dist.all_gather_into_tensor(allc, torch.tensor(mine, dtype=torch.int64))
        counts = np.ascontiguousarray(allc.numpy().astype(np.uint64))
        pbase = np.zeros(world, np.uint64)
        obase = np.zeros(world, np.uint64)
        tp, to = C.c_uint64(), C.c_uint64()
        rc = self.H.eg3d_host_gather_plan(world, D.np_ptr(counts, C.c_uint64), D.np_ptr(pbase, C.c_uint64),
                                          D.np_ptr(obase, C.c_uint64), C.byref(tp), C.byref(to))
        if rc != 0:
            return None, rc
        tp, to = int(tp.value), int(to.value)
        whole = {"X": np.zeros((tp, 3), np.float32), "obs_off": np.zeros(tp + 1, np.uint64),
                 "key": np.zeros((tp, 4), np.uint32), "obs_view": np.zeros(to, np.int32), "obs_pl": np.zeros(to, np.uint32),
                 "obs_seg": np.zeros(to, np.uint32), "obs_xy": np.zeros((to, 2), np.float32)}
        whole_c = D.EdgePointsArrays(whole)
        whole_c.c.n_points, whole_c.c.n_obs = tp, to
        dtypes = {"X": np.float32, "obs_off": np.uint64, "key": np.uint32, "obs_view": np.int32, "obs_pl": np.uint32,
                  "obs_seg": np.uint32, "obs_xy": np.float32}
        for r in range(world):
            np_r, no_r = int(counts[3 * r]), int(counts[3 * r + 1])
            part = {}
            for name, per, per_point in FIELDS:
                n_el = np_r if per_point else no_r
                nbytes = n_el * per
                if r == rank:
                    a = np.ascontiguousarray(local[name] if name != "obs_off" else local[name][:np_r], dtypes[name])
                    buf = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()) if nbytes else torch.zeros(0, dtype=torch.uint8)
                else:
                    buf = torch.empty(nbytes, dtype=torch.uint8)
                if nbytes:
                    dist.broadcast(buf, src=r)
                part[name] = buf.numpy().view(dtypes[name]) if nbytes else np.zeros(0, dtypes[name])
            part["obs_off"] = np.concatenate([part["obs_off"], np.array([no_r], np.uint64)])  # EdgePointsArrays wants the sentinel
            part_c = D.EdgePointsArrays(part)
            part_c.c.n_points, part_c.c.n_obs = np_r, no_r
            rc = self.H.eg3d_host_gather_place(C.byref(part_c.c), int(pbase[r]), int(obase[r]), C.byref(whole_c.c))
            if rc != 0:
                return None, rc
        out = dict(whole_c.a)
        out["obs_off"][tp] = to
        out["X"] = out["X"].reshape(-1, 3)
        out["key"] = out["key"].reshape(-1, 4)
        out["obs_xy"] = out["obs_xy"].reshape(-1, 2)
        out["n_points"], out["n_obs"] = tp, to
        return out, 0


    # ---- the exchanges of the dedup in phases, as RcclCloudGather has them ----
    def exscan_points(self, n_points):
        """(points of the lower ranks, points of all ranks, rc): one all-gather of the counts."""
        allc = torch.empty(self.world, dtype=torch.int64)
        self.dist.all_gather_into_tensor(allc, torch.tensor([int(n_points)], dtype=torch.int64))
        counts = [int(x) for x in allc.tolist()]
        if sum(counts) >= 0xFFFFFFFF:
            return 0, sum(counts), -1
        return sum(counts[:self.rank]), sum(counts), 0

    def allreduce_claims(self, first_np):
        """first_np (a contiguous uint32 claim map, e.g. HostShard.dedup_claims()) becomes the minimum over the ranks, in
        place. None: this rank has no usable map. First the agreement round of eg3d_allreduce_claims — any rank without a
        map: -4 on every rank; ranks whose maps differ in size: -1 on every rank — then the reduction. gloo has no uint32,
        and 0xFFFFFFFF read as int32 is -1, which a minimum would prefer to every claim: the map is reduced as an int64
        copy and written back."""
        import numpy as np
        mine = -1 if first_np is None else int(first_np.size)
        allc = torch.empty(self.world, dtype=torch.int64)
        self.dist.all_gather_into_tensor(allc, torch.tensor([mine], dtype=torch.int64))
        sizes = allc.tolist()
        if any(x < 0 for x in sizes):
            return -4
        if any(x != sizes[0] for x in sizes):
            return -1
        if first_np.dtype != np.uint32 or not first_np.flags["C_CONTIGUOUS"]:
            raise ValueError("a contiguous uint32 map is needed")
        t = torch.from_numpy(first_np.astype(np.int64).reshape(-1))
        if self.world > 1 and t.numel():
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN)
        first_np.reshape(-1)[:] = t.numpy().astype(np.uint32)
        return 0


class HostShard:
    """A rank's shard on host arrays with the calls of api.Context that dedup_filter_then_gather makes, on the host
    statements: eg3d_host_dedup_claim / _keep (include/eg3d_host_dedup_phases.h) and cloudnp.np_compact. The
    Gauss-Newton verdict comes from the caller: gn_filter(cloud dict, gn_max_mse, legacy_abs) -> (X_new [n, 3] float32,
    inlier [n] uint8) — the product has no host form of that filter; the tests pass the CPU oracle's. A run on
    HostCloudGather (gloo) is then the same sequence as a run on the device and RcclCloudGather."""

    def __init__(self, cloud, n_views, width, height, gn_filter):
        import types
        self.n_views, self.width, self.height, self.gn_filter = int(n_views), int(width), int(height), gn_filter
        self.view = types.SimpleNamespace(n_points=int(cloud["n_points"]), n_obs=int(cloud["n_obs"]), complete=1, arrays=cloud)
        self.first = None

    def last_device_output(self):
        return self.view

    def dedup_claims(self):
        from . import host
        if self.first is None:
            self.first = host.dedup_empty_claims(self.n_views, self.width, self.height)
        return self.first

    def dedup_claim(self, view, index_base=0, reset=False):
        from . import host
        if reset:
            self.first = None
        host.dedup_claim(view.arrays, self.n_views, self.width, self.height, self.dedup_claims(), index_base)

    def dedup_keep(self, view, index_base=0):
        from . import host
        if self.first is None:
            raise ValueError("nothing was claimed")
        return host.dedup_keep(view.arrays, self.n_views, self.width, self.height, self.first, index_base)

    def gn_filter_device(self, view, keep=None, gn_max_mse=2.25, legacy_abs=False):
        import numpy as np
        from .cloudnp import np_compact
        c, n = view.arrays, view.n_points
        sel = np.ones(n, bool) if keep is None else np.asarray(keep).astype(bool)
        X_out, inlier = np.array(c["X"], np.float32).reshape(-1, 3).copy(), np.zeros(n, np.uint8)
        if sel.any():   # a masked-out point is no inlier and keeps its X, as on the device
            Xs, inl = self.gn_filter(np_compact(c, sel), gn_max_mse, legacy_abs)
            X_out[sel], inlier[sel] = Xs, inl
        k = np.diff(np.asarray(c["obs_off"]).astype(np.int64))[inlier.astype(bool)]
        hist = np.bincount(k[k <= self.n_views], minlength=self.n_views + 1).astype(np.int64)
        return X_out, inlier, hist, int(inlier.sum()), 0.0

    def compact_device(self, view, keep=None, X_new=None, min_obs=-1):
        import numpy as np
        from .cloudnp import np_compact
        out = np_compact(view.arrays, np.ones(view.n_points, np.uint8) if keep is None else keep, X_new, min_obs)
        return out


# ---- the filter stage over ranks: each rank filters the shard it already holds in HBM, only the survivors travel ----
def observation_threshold(hist, n_views, forced_min_filter=-1, count=None):
    """The rule of eg3d_host_observation_filter (host/post_steps.cpp) on a histogram by list length: hist[k] = points with
    k observations, k = 0 .. n_views; `count` = all points, those with longer lists included (default: the histogram's
    sum). The median bin, then max(3, median // 2 - 1); forced_min_filter > -1 overrides. A point is kept with MORE
    observations than the result."""
    hist = [int(h) for h in hist]
    if len(hist) != n_views + 1:
        raise ValueError("the histogram needs n_views + 1 entries")
    count = sum(hist) if count is None else int(count)
    acc, median = 0, n_views
    for m in range(n_views):
        acc += hist[m + 1]
        if acc >= count // 2:
            median = m
            break
    threshold = max(3, median // 2 - 1)
    return int(forced_min_filter) if forced_min_filter > -1 else threshold


def global_observation_threshold(dist, local_hist, n_views, forced_min_filter=-1, base_hist=None, local_count=None):
    """Sum-all-reduce of the ranks' int64 histograms (Context.gn_filter_device returns one per shard), then the threshold
    of the whole cloud, the same on every rank. base_hist: the caller's SfM points ([n_views + 1], the same on every
    rank: added once). local_count: this rank's inliers when some have more than n_views observations (default: the
    histogram's sum). dist = torch.distributed, or None for a single process."""
    v = [int(h) for h in local_hist]
    if len(v) != n_views + 1:
        raise ValueError("the histogram needs n_views + 1 entries")
    t = torch.tensor(v + [sum(v) if local_count is None else int(local_count)], dtype=torch.int64)
    if dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
        if dist.get_backend() == "nccl":
            t = t.cuda()
        dist.all_reduce(t)
        t = t.cpu()
    hist, count = t[:-1].tolist(), int(t[-1])
    if base_hist is not None:
        if len(base_hist) != n_views + 1:
            raise ValueError("base_hist needs n_views + 1 entries")
        hist = [h + int(b) for h, b in zip(hist, base_hist)]
        count += sum(int(b) for b in base_hist)
    return observation_threshold(hist, n_views, forced_min_filter, count)


def filter_then_gather(ctx, gather, dist, gn_max_mse=2.25, legacy_abs=False, forced_min_filter=-1, base_hist=None, keep=None):
    """The end of a multi-GPU run without a gathered intermediate: (1) Context.gn_filter_device on this rank's
    device-only cloud (keep: optional device mask of the shard — Context.dedup_device gives the dedup mask of a shard on
    its own or of a gathered / concatenated cloud; the dedup of a SHARDED cloud against the other ranks' shards, which
    exchanges the claim maps, is dedup_filter_then_gather below), (2) the global threshold,
    (3) Context.compact_device of the inliers above it, new X in place, (4) gather.allgather of the compacted shard.
    Returns (DeviceEdgePoints of all ranks' survivors, rc of the gather, threshold). Every rank must call it."""
    cloud = ctx.last_device_output()
    if not cloud.complete:
        raise RuntimeError("the device view does not hold the whole cloud of the last call")
    # (inliers with more observations than views sit in no bin: n_inl counts them too)
    X_out, inlier, hist, n_inl, _ = ctx.gn_filter_device(cloud, keep, gn_max_mse, legacy_abs)
    thr = global_observation_threshold(dist, hist, ctx.n_views, forced_min_filter, base_hist, local_count=n_inl)
    shard = ctx.compact_device(cloud, inlier, X_out, thr)
    out, rc = gather.allgather(shard)
    X_out.free()
    inlier.free()
    return out, rc, thr


def dedup_filter_then_gather(ctx, gather, dist, run_base=0, gn_max_mse=2.25, legacy_abs=False, forced_min_filter=-1,
                             base_hist=None, reset=None):
    """The reference-exact end of a sharded step, the raw cloud never travelling: the reference dedups BEFORE it filters,
    and a shard can only be deduplicated against the claims of all ranks. On this rank's device-only cloud:
      (1) gather.exscan_points: the shard's index base = the points of the lower ranks (rank order = seed order);
      (2) ctx.dedup_claim with run_base + that base (run_base: the points of the earlier steps of the run; reset, default
          run_base == 0, empties the map first — without it the claims of the earlier steps, already reduced, stand);
      (3) gather.allreduce_claims: the element-wise minimum of the ranks' claim maps, in place;
      (4) ctx.dedup_keep: the shard's part of the mask of the whole cloud;
      (5) ctx.gn_filter_device with that mask; (6) global_observation_threshold; (7) ctx.compact_device;
      (8) gather.allgather of the survivors.
    Every rank ends with eg3d_dedup_resident(with_filter) of the concatenation of the shards. ctx / gather: an api.Context
    with an RcclCloudGather, or a HostShard with a HostCloudGather. Returns (cloud of all ranks' survivors, rc, threshold);
    a rank whose claim fails still takes part in (3), every rank then gets (None, -4, None) and none blocks; ranks that
    disagree on the rig get (None, -1, None). Every rank must call it."""
    cloud = ctx.last_device_output()
    if not cloud.complete:
        raise RuntimeError("the device view does not hold the whole cloud of the last call")
    base, total, rc = gather.exscan_points(int(cloud.n_points))
    if rc != 0:
        return None, rc, None
    index_base, claimed = int(run_base) + base, True
    try:
        ctx.dedup_claim(cloud, index_base, reset=(int(run_base) == 0) if reset is None else bool(reset))
    except Exception:   # this rank's verdict travels in the agreement round: the peers must not wait for its payload
        claimed = False
    mine = None if not claimed else (ctx if isinstance(gather, RcclCloudGather) else ctx.dedup_claims())
    rc = gather.allreduce_claims(mine)
    if rc != 0:
        return None, rc, None
    keep, _ = ctx.dedup_keep(cloud, index_base)
    # (inliers with more observations than views sit in no bin: n_inl counts them too)
    X_out, inlier, hist, n_inl, _ = ctx.gn_filter_device(cloud, keep, gn_max_mse, legacy_abs)
    thr = global_observation_threshold(dist, hist, ctx.n_views, forced_min_filter, base_hist, local_count=n_inl)
    shard = ctx.compact_device(cloud, inlier, X_out, thr)
    out, rc = gather.allgather(shard)
    for a in (keep, X_out, inlier):
        if hasattr(a, "free"):
            a.free()
    return out, rc, thr


def replay_merge_ranks(target, dist, graph, n_points, n_pairs=0, reset=True):
    """The matches manager of a sharded run, the raw cloud never travelling: every rank replays its own shard (rank order =
    seed order; a shard is made of whole chains, as a seed range is) and contributes the GRAPH — `graph`: the dict that
    Context.replay_device, Context.replay_accumulate or host.replay_matches return — with the shard's point count and,
    for the totals, its pairs. The graphs are gathered (plain arrays: 12 + 8 bytes per node, 8 per polyline, at most one
    interval per scene vertex; dist.all_gather_object, no RCCL code of this library) and every rank folds them in rank order
    into `target` — an api.Context (its accumulator, eg3d_replay_merge_graph; reset starts a new graph with rank 0's) or a
    host.ReplayState (eg3d_host_replay_state_merge_graph; an existing state is continued). Every rank ends with the same
    graph, byte for byte what the replay of the concatenation of all shards' clouds builds, and returns it as a dict. A
    refused graph raises on every rank alike (all fold the same graphs). Every rank must call it."""
    world = dist.get_world_size()
    mine = {k: (v if hasattr(v, "dtype") else int(v)) for k, v in graph.items()}
    parts = [None] * world
    dist.all_gather_object(parts, (mine, int(n_points), int(n_pairs)))
    out = None
    for r, (g, n, pairs) in enumerate(parts):
        if hasattr(target, "replay_merge"):
            out = target.replay_merge(g, n, pairs, reset=bool(reset) and r == 0, materialise=(r == world - 1))[0]
        else:
            target.merge(g, n)
    return out if out is not None else target.graph()
