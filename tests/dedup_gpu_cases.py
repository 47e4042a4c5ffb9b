"""What the GPU tests of the device dedup share: the C2 cloud of one DLT form left in HBM by a device-only match, its
host copy, its host dedup mask and the oracle's filter, and the host statement of the observation threshold."""
import ctypes as C

import numpy as np

import dedup_cases as dc
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host


class C2Cloud:
    def __init__(self, rows):
        assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
        self.s = host.Synth(2)
        self.ctx = api.Context(self.s.scene)
        r = self.ctx.match_refpoints(self.s.seeds, device_only=True)
        self.dev = self.ctx.last_device_output()
        assert self.dev.complete == 1 and int(self.dev.n_points) == r["n_points"] > 1000
        self.cloud = self.ctx.fetch_device_output()
        self.n = self.cloud["n_points"]
        sc = self.s.scene.contents
        self.V, self.W, self.H = self.s.n_views, int(sc.width), int(sc.height)
        self.dedup = dc.host_mask(self.cloud, self.V, self.W, self.H)
        self.mse = 2.25   # the reference's default

    def oracle_filter(self, cloud, mse):
        from oracle import binding as ob
        return ob.Oracle(self.s.scene).gn_filter(cloud["X"], cloud["obs_off"].astype(np.uint32), cloud["obs_view"],
                                                 cloud["obs_xy"], mse, legacy_abs=False, nthreads=16)

    def view(self, n):
        """The first n points as a caller-built device view."""
        d = D.DeviceEdgePoints()
        C.memmove(C.byref(d), C.byref(self.dev), C.sizeof(d))
        d.n_points, d.n_obs = n, int(self.cloud["obs_off"][n])
        return d


def host_threshold(V, k, inl, forced, sfm_k=None):
    """eg3d_host_observation_filter on [SfM points] + [the cloud]: (threshold, surviving mask of the cloud)."""
    sfm_k = np.zeros(0, np.int64) if sfm_k is None else sfm_k
    off = np.concatenate([[0], np.cumsum(np.concatenate([sfm_k, k]))]).astype(np.uint32)
    mask = np.concatenate([np.ones(len(sfm_k), np.uint8), np.asarray(inl, np.uint8)])
    thr = host.lib().eg3d_host_observation_filter(V, D.np_ptr(off, C.c_uint32), len(mask), len(sfm_k), forced,
                                                  D.np_ptr(mask, C.c_uint8))
    return thr, mask[len(sfm_k):]
