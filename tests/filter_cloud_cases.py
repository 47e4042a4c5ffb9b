"""Hand-built device clouds for the filter stage on a device-resident cloud: the inputs that take the branches of
k5_gn_filter<eg3d_off_t, false> and of the k6_compact_* kernels which a matched cloud never reaches. A plain module (no
GPU needed to import it): tests/test_filter_cloud_cases.py checks with the oracle alone that every case reaches what it
is for, tests/test_gpu_filter_device_paths.py runs the kernels on them.

A case is (rig, blocks): `blocks` in the format of _k5_lists, 256 points (one k5_gn_filter block) per entry. A block
is "light" when its lists hold at most K5_OBS_CAP = 2816 observations (staged in LDS where the rig has at most
K5_VIEW_CAP = 256 views) and "heavy" otherwise (operands from HBM). The final list lengths:

rig16 (host.Synth(5), 16 views), 3 * 256 + 101 = 869 points (101 % 64 = 37), blocks in this order:
    light   [0, 1, 2, 3, 10, 16, 17, 20, 63, 64, 65] twice, then [0, 1, 2, 3, 5, 8] repeated
    heavy   [0, 1, 2, 3, 10, 16, 17, 20, 63, 64, 65] repeated (about 6 000 observations)
    light   [3, 0, 2, 1, 10, 4, 16, 6, 17, 0, 20, 5] repeated
    partial the first 101 points of [65, 0, 64, 1, 63, 2, 3, 20, 17, 16, 10] repeated (heavy as a whole block; what is
            left of it is light)
    Both verdicts are asserted at 2, 3, 10, 16, 17, 20, 63, 64, 65. Lengths 0 and 1 are dropped from that condition: the
    normal matrix of fewer than two observations is singular and the oracle rejects every such point (only the legacy
    abs() accepts a single observation whose first mse is below 1, unmoved).
rig256, rig257 (default_config(4) with n_views set, n_seeds 10, n_curves 20), 512 points:
    light   [2, 63, 64, 65, 256, 257, 258] twice, then [2, 3] repeated
    heavy   [2, 63, 64, 65, 256, 257, 258] repeated (about 35 000 observations)
    Both verdicts at every one of the seven lengths. Over-long: 257 and 258 on rig256, 258 on rig257.
threshold16 (host.Synth(5)), 1024 points, observation noise 0.3 .. 1.7 px:
    light   [8, 8, 8, 7, 8, 20, 8, 5, 8, 16] repeated
    heavy   [16, 20, 20, 20, 20] repeated, three such blocks
    About 880 inliers, 550 of them of length 20 > 16 views: with them in the count and in no bin the median loop of the
    observation filter runs off the end (threshold 16 // 2 - 1 = 7); binned at V the median is bin 16 (threshold 6);
    left out of the count the median is bin 8 (threshold 3)."""
import ctypes as C

import numpy as np

from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import host

K5_BLOCK, K5_OBS_CAP, K5_VIEW_CAP = 256, 2816, 256
K6_SCAN_TRIP = 1024 * 256      # points one trip of k6_compact_scan covers (1024 block totals of 256 points)
GN_MAX_MSE = 2.25              # the reference's default


def _k5_lists(s, rng, lengths_per_block, sigma=(0.3, 2.5)):
    """Points of the rig of `s` with the given list lengths, 256 points (one k5_gn_filter block) per entry: views drawn
    without repetition while the rig has enough, observations = projection + noise of 0.3 .. 2.5 px (a point's own level:
    both sides of the mse threshold), start = true point + 1.5 per axis."""
    P = s.scene_np()["cam_P"].reshape(-1, 4, 4)[:, :3, :].astype(np.float64)
    V = len(P)
    Xt, _, _, _ = s.points(256 * len(lengths_per_block))
    Xt = Xt.astype(np.float64)
    ks = np.concatenate([np.resize(np.asarray(b), 256) for b in lengths_per_block]).astype(np.int64)
    views = []
    for k in ks:
        v = rng.choice(V, min(int(k), V), replace=False)
        views.append(np.concatenate([v, rng.integers(0, V, int(k) - len(v))]) if k > V else v)
    off = np.concatenate([[0], np.cumsum(ks)]).astype(np.uint32)
    view = np.concatenate(views).astype(np.int32)
    pid = np.repeat(np.arange(len(ks)), ks)
    h = np.einsum("nij,nj->ni", P[view], np.concatenate([Xt[pid], np.ones((len(pid), 1))], 1))
    sigma = rng.uniform(sigma[0], sigma[1], len(ks))[pid][:, None]
    xy = (h[:, :2] / h[:, 2:3] + rng.normal(0, 1, (len(pid), 2)) * sigma).astype(np.float32)
    X0 = (Xt + rng.normal(0, 1.5, Xt.shape)).astype(np.float32)
    return X0, off, view, xy


_RIG16_LENGTHS = [0, 1, 2, 3, 10, 16, 17, 20, 63, 64, 65]
_WIDE_LENGTHS = [2, 63, 64, 65, 256, 257, 258]


def _fill(head, tail):
    """256 lengths: `head`, then `tail` repeated."""
    return list(head) + list(np.resize(np.asarray(tail), 256 - len(head)))


# name -> (rig, blocks, points kept (None: all), noise range, the lengths with both verdicts)
_SPECS = {
    "rig16": (5, [_fill(_RIG16_LENGTHS * 2, [0, 1, 2, 3, 5, 8]), _RIG16_LENGTHS, [3, 0, 2, 1, 10, 4, 16, 6, 17, 0, 20, 5],
                  [65, 0, 64, 1, 63, 2, 3, 20, 17, 16, 10]], 3 * 256 + 101, (0.3, 2.5), _RIG16_LENGTHS[2:]),
    "rig256": (256, [_fill(_WIDE_LENGTHS * 2, [2, 3]), _WIDE_LENGTHS], None, (0.3, 2.5), _WIDE_LENGTHS),
    "rig257": (257, [_fill(_WIDE_LENGTHS * 2, [2, 3]), _WIDE_LENGTHS], None, (0.3, 2.5), _WIDE_LENGTHS),
    "threshold16": (5, [[8, 8, 8, 7, 8, 20, 8, 5, 8, 16]] + [[16, 20, 20, 20, 20]] * 3, None, (0.3, 1.7), [8, 16, 20]),
}
K5_CASES = tuple(_SPECS)
LISTED_LENGTHS = {"rig16": _RIG16_LENGTHS, "rig256": _WIDE_LENGTHS, "rig257": _WIDE_LENGTHS, "threshold16": [5, 7, 8, 16, 20]}
_RIGS, _CASES = {}, {}


def rig(which):
    """host.Synth(5) for which == 5, else the config-4 rig of `which` views; created once per process."""
    if which not in _RIGS:
        if which == 5:
            _RIGS[which] = host.Synth(5)
        else:
            cfg = host.default_config(4)
            cfg.n_views, cfg.n_seeds, cfg.n_curves = which, 10, 20
            _RIGS[which] = host.Synth(cfg)
            assert _RIGS[which].n_views == which
    return _RIGS[which]


class Case:
    """One named K5 case: the host arrays (obs_off uint32 with its sentinel, as the oracle takes them) and, computed once
    per abs() behaviour and DLT mode, the oracle's verdicts and positions. Nothing here is modified after creation."""

    def __init__(self, name):
        which, blocks, n, sigma, both = _SPECS[name]
        self.name, self.rig_id, self.s = name, which, rig(which)
        self.V = self.s.n_views
        X, off, view, xy = _k5_lists(self.s, np.random.default_rng(1000 + which + len(name)), blocks, sigma)
        if n is not None:      # the last block is partial: cut the arrays
            X, off = X[:n], off[:n + 1]
            view, xy = view[:int(off[n])], xy[:int(off[n])]
        self.X, self.off, self.view, self.xy = (np.ascontiguousarray(a) for a in (X, off, view, xy))
        self.n, self.n_obs = len(X), int(off[-1])
        self.k = np.diff(off.astype(np.int64))
        self.per_block = np.add.reduceat(self.k, np.arange(0, self.n, K5_BLOCK))
        self.heavy = self.per_block > K5_OBS_CAP                    # blocks whose slice does not fit the staging area
        self.staged = ~self.heavy & (self.V <= K5_VIEW_CAP)         # what k5_gn_filter decides per block
        self.both_verdicts = both
        self.mse = GN_MAX_MSE
        self._ref = {}
        for a in (self.X, self.off, self.view, self.xy, self.k):
            a.setflags(write=False)

    def oracle(self, legacy=False):
        """(X_out, inlier) of Oracle.gn_filter on the case's arrays."""
        from oracle import binding as ob
        key = (bool(legacy), int(ob.lib().orc_get_dlt_rows()))
        if key not in self._ref:
            Xr, ir = ob.Oracle(self.s.scene).gn_filter(self.X, self.off, self.view, self.xy, self.mse, legacy_abs=legacy,
                                                       nthreads=16)
            Xr.setflags(write=False)
            ir.setflags(write=False)
            self._ref[key] = (Xr, ir)
        return self._ref[key]

    def first_heavy(self):
        return int(np.flatnonzero(self.heavy)[0])

    def first_light(self):
        return int(np.flatnonzero(~self.heavy)[0])

    def coverage(self, inlier=None):
        """One line: blocks staged / not staged, points per listed length, inlier share, overflow-bin count."""
        txt = "%s: %d points, %d obs, V %d, blocks staged %d / not staged %d (heavy %d); points per length %s" % (
            self.name, self.n, self.n_obs, self.V, int(self.staged.sum()), int((~self.staged).sum()), int(self.heavy.sum()),
            " ".join("%d:%d" % (k, (self.k == k).sum()) for k in LISTED_LENGTHS[self.name]))
        if inlier is not None:
            inl = np.asarray(inlier) != 0
            txt += "; inliers %.3f, overflow bin %d" % (inl.mean(), int((inl & (self.k > self.V)).sum()))
        return txt


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


MASKS = ("random50", "block_off", "wave_off", "ones", "zeros")


def mask(c, name):
    """The keep masks of the GPU tests (uint8, one per point) on case `c`: a random half; one whole block zeroed (the
    first light one); one whole wavefront (64 consecutive points) of the first heavy block zeroed; all ones; all zeros."""
    m = np.ones(c.n, np.uint8)
    if name == "random50":
        m = (np.random.default_rng(50 + c.n).random(c.n) < 0.5).astype(np.uint8)
    elif name == "block_off":
        b = c.first_light()
        m[b * K5_BLOCK:(b + 1) * K5_BLOCK] = 0
    elif name == "wave_off":
        b = c.first_heavy()
        m[b * K5_BLOCK + 64:b * K5_BLOCK + 128] = 0
    elif name == "zeros":
        m[:] = 0
    else:
        assert name == "ones", name
    return m


def lone_empty_between_long(c):
    """A keep mask with three survivors that sit in one wavefront of the first heavy block: a list of 64 or more, an EMPTY
    list, a list of 64 or more. None when the case has no such triple."""
    b = c.first_heavy()
    for w0 in range(b * K5_BLOCK, min((b + 1) * K5_BLOCK, c.n), 64):
        kw = c.k[w0:w0 + 64]
        long_ = np.flatnonzero(kw >= 64)
        for j in np.flatnonzero(kw == 0):
            if (long_ < j).any() and (long_ > j).any():
                m = np.zeros(c.n, np.uint8)
                m[[w0 + long_[long_ < j][-1], w0 + j, w0 + long_[long_ > j][0]]] = 1
                return m
    return None


def host_cloud(X, off, view, xy):
    """The cloud dict np_compact / same_cloud take (obs_off uint64 with its sentinel) over the four filter arrays;
    obs_pl, obs_seg and key are distinct running numbers, so a misplaced row shows in a comparison."""
    n, m = len(X), int(off[-1])
    return {"n_points": n, "n_obs": m, "X": np.ascontiguousarray(X, np.float32).reshape(n, 3),
            "obs_off": np.ascontiguousarray(off).astype(np.uint64), "key": (np.arange(4 * n, dtype=np.uint32) + 5).reshape(n, 4),
            "obs_view": np.ascontiguousarray(view, np.int32), "obs_pl": np.arange(m, dtype=np.uint32) + 1000,
            "obs_seg": np.arange(m, dtype=np.uint32) * 3 + 7, "obs_xy": np.ascontiguousarray(xy, np.float32).reshape(m, 2)}


def device_cloud(ctx, X, off, view, xy):
    """Uploads a hand-built cloud: (DeviceEdgePoints with complete = 1, the DeviceArrays that keep its memory alive, the
    host dict of host_cloud). off: n_points + 1 offsets; the device gets the first n_points as uint64 words, WITHOUT the
    sentinel, and n_obs in the struct."""
    cloud = host_cloud(X, off, view, xy)
    n = cloud["n_points"]
    keepalive = {"X": ctx.upload(cloud["X"]), "obs_off": ctx.upload(cloud["obs_off"][:n])}
    for name in ("obs_view", "obs_pl", "obs_seg", "obs_xy", "key"):
        keepalive[name] = ctx.upload(cloud[name])
    d = D.DeviceEdgePoints()
    d.n_points, d.n_obs, d.complete = n, cloud["n_obs"], 1
    for name, a in keepalive.items():
        setattr(d, name, a.ptr)
    return d, keepalive, cloud


def same_view(dev):
    """A copy of a DeviceEdgePoints struct (to point single members elsewhere)."""
    d = D.DeviceEdgePoints()
    C.memmove(C.byref(d), C.byref(dev), C.sizeof(d))
    return d


def host_threshold(V, k, inl, forced=-1):
    """eg3d_host_observation_filter on the cloud alone: (threshold, surviving mask)."""
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.uint32)
    m = np.array(inl, np.uint8)
    thr = host.lib().eg3d_host_observation_filter(V, D.np_ptr(off, C.c_uint32), len(m), 0, forced, D.np_ptr(m, C.c_uint8))
    return thr, m


def scan_cloud(n):
    """The arrays of a cloud for the compaction alone (no rig; K5 is never run on it): n points whose list lengths cycle
    through 0, 1, 2, 3, everything else arbitrary."""
    rng = np.random.default_rng(n)
    k = np.arange(n, dtype=np.int64) % 4
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.uint64)
    m = int(off[-1])
    return (rng.standard_normal((n, 3)).astype(np.float32), off, rng.integers(0, 16, m).astype(np.int32),
            rng.standard_normal((m, 2)).astype(np.float32))
