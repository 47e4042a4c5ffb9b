"""Tables for include/eg3d_colour.h, shared by the CPU tests (tests/test_colour_host.py: the host statement against
tests/colour_ref.py) and the GPU tests (tests/test_gpu_colour.py: K15 against the host statement). Rows are the smallest at
which each piece can go wrong.

Images of a rig of V views (V >= 15): view v < V - 3 has size SIZES[v % 6] (W x H: 1x1, 1x5, 5x1, 2x2, 3x2, 7x5), a 0/255
checkerboard (every channel its own phase) when (v // 6) is even and seeded bytes when it is odd; view V - 3 is the 6x2
`ties` image (columns 0, 1, 2, 254, 255, 0 in every channel); view V - 2 a seeded 2x2 image for the 32 767-observation
point; view V - 1 has NO image and only the refusal rows name it."""
import functools

import numpy as np

SIZES = ((1, 1), (1, 5), (5, 1), (2, 2), (3, 2), (7, 5))   # (W, H)
MAX_OBS = 32767


@functools.lru_cache(maxsize=None)
def images(V):
    assert V >= 15
    rng = np.random.default_rng(1500 + V)
    out = []
    for v in range(V - 3):
        W, H = SIZES[v % 6]
        if (v // 6) % 2 == 0:
            yy, xx = np.mgrid[0:H, 0:W]
            im = np.stack([(((xx + yy + ch) % 2) * 255) for ch in range(3)], axis=2).astype(np.uint8)
        else:
            im = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        out.append(im)
    ties = np.array([0, 1, 2, 254, 255, 0], np.uint8)
    out.append(np.ascontiguousarray(np.broadcast_to(ties[None, :, None], (2, 6, 3))))
    out.append(rng.integers(0, 256, (2, 2, 3), dtype=np.uint8))
    out.append(None)
    return tuple(out)


def ties_view(V):
    return V - 3


def big_view(V):
    return V - 2


def empty_view(V):
    return V - 1


class Cloud:
    """Points as lists of (view, x, y) -> the CSR arrays both entry points take."""

    def __init__(self, points, keep=None):
        rows = [len(p) for p in points]
        self.n = len(points)
        self.obs_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint32)
        flat = [o for p in points for o in p]
        self.obs_view = np.array([o[0] for o in flat] or [0], np.int32)[:len(flat)]
        self.obs_xy = np.array([[o[1], o[2]] for o in flat] or [[0, 0]], np.float32)[:len(flat)].reshape(-1, 2)
        self.keep = None if keep is None else np.asarray(keep, np.uint8)

    def args(self):
        return self.obs_off, self.obs_view, self.obs_xy

    def device_offsets(self):
        """64-bit offsets without the sentinel, as a device cloud carries them."""
        return self.obs_off[:-1].astype(np.uint64)


def _axis(L):
    """Coordinates along an axis of length L: integers, the last pixel (its +1 neighbour reflects to L - 2), inside
    (L - 1, L), at and beyond L, several periods out on both sides, and inside (-1, 0), where truncation toward zero gives a
    negative weight."""
    return [0.0, float(L - 1), L - 1 + 0.5, float(L), L + 0.25, 3 * L + 0.25, -2 * L - 0.75, -0.5, -0.25, -1.0, 0.75]


@functools.lru_cache(maxsize=None)
def main_points(V):
    ims = images(V)
    pts = []
    for v in range(V - 3):
        H, W = ims[v].shape[:2]
        for x in _axis(W):
            pts.append([(v, x, 0.0)])
        for y in _axis(H):
            pts.append([(v, 0.0, y)])
        pts.append([(v, -0.5, -0.5)])                       # negative weights on both axes
        pts.append([(v, W - 0.5, H - 0.5)])
        pts.append([(v, 3 * W + 0.25, -2 * H - 0.75)])
    t, b = ties_view(V), big_view(V)
    # exact ties at a = 0.5: 0|1 -> 0, 1|2 -> 2, 254|255 -> 254 (ties to even)
    pts += [[(t, 0.5, 0.0)], [(t, 1.5, 0.0)], [(t, 3.5, 0.0)], [(t, 0.5, 0.5)]]
    # s < 0 and s > 255.5 on a checkerboard row (view 4 is the 3x2 checkerboard): the low byte of the rounded int
    pts += [[(4, -0.5, 0.0)], [(4, -0.5, 1.0)], [(4, -0.75, -0.75)]]
    # just below 1e7: FP32 has no fraction left (view 5: 7x5)
    below = float(np.nextafter(np.float32(1e7), np.float32(0)))
    pts += [[(5, below, 1.0)], [(5, 2.0, -below)]]
    # the mix: two whose sum is odd (255 + 254 -> 254), thirds (255 + 254 + 254 -> 254; 1 + 1 + 2 -> 1), one view twice,
    # several views, none
    pts.append([(t, 4.0, 0.0), (t, 3.0, 0.0)])
    pts.append([(t, 4.0, 0.0), (t, 3.0, 1.0), (t, 3.0, 0.0)])
    pts.append([(t, 1.0, 0.0), (t, 1.0, 1.0), (t, 2.0, 0.0)])
    pts.append([(5, 1.25, 2.5), (5, 1.25, 2.5)])
    pts.append([(11, 6.5, 4.5), (3, 0.5, 0.5), (9, 1.0, -0.5), (t, 2.5, 0.25), (0, 7.0, -3.0)])
    pts.append([])
    # 32 767 observations, all in one 2x2 image
    rng = np.random.default_rng(1515)
    xy = rng.uniform(-3.0, 5.0, (MAX_OBS, 2)).astype(np.float32)
    pts.append([(b, float(p[0]), float(p[1])) for p in xy])
    pts.append([(6, 0.0, 0.0)])
    return pts


def main(V):
    return Cloud(main_points(V))


def main_masked(V):
    """drops the first, the last and a middle point (and every seventh)"""
    pts = main_points(V)
    keep = np.ones(len(pts), np.uint8)
    keep[[0, len(pts) // 2, len(pts) - 1]] = 0
    keep[3::7] = 0
    return Cloud(pts, keep)


def _small(V, bad, keep=None):
    """three points, the middle one carrying the row under test"""
    return Cloud([[(5, 1.5, 2.5)], bad, [(3, 0.25, 0.75), (4, 1.0, 1.0)]], keep)


def refusals(V):
    """{name: Cloud}: each is refused, alone, with EG3D_ERR_ARG"""
    out = {}
    for name, val in (("nan", float("nan")), ("inf", float("inf")), ("1e7", 1e7), ("minus_1e7", -1e7), ("minus_inf", float("-inf"))):
        out[name + "_x"] = _small(V, [(5, val, 1.0)])
        out[name + "_y"] = _small(V, [(5, 1.0, val), (5, 0.0, 0.0)])
    out["view_minus_1"] = _small(V, [(-1, 0.0, 0.0)])
    out["view_V"] = _small(V, [(V, 0.0, 0.0)])
    out["view_without_image"] = _small(V, [(empty_view(V), 0.0, 0.0)])
    d = _small(V, [(5, 0.0, 0.0)])
    d.obs_off = np.array([0, 2, 1, 4], np.uint32)
    out["descending_offsets"] = d
    out["list_of_32768"] = Cloud([[(5, 1.0, 1.0)], [(big_view(V), 0.5, 0.5)] * (MAX_OBS + 1)])
    return out


def dropped_bad(V):
    """refused observations on points the mask drops: NOT a refusal"""
    pts = [[(5, 1.5, 2.5)], [(5, float("nan"), 1.0)], [(V, 0.0, 0.0)], [(3, 0.25, 0.75), (4, 1.0, 1.0)], [(empty_view(V), 1.0, 1.0)],
           [(big_view(V), 0.5, 0.5)] * (MAX_OBS + 1), [(2, 1e7, 0.0)]]
    return Cloud(pts, [1, 0, 0, 1, 0, 0, 0])


def valid_probe(V):
    """the valid call made after each refusal"""
    return _small(V, [(9, 1.0, 0.5), (ties_view(V), 3.5, 0.0)])


def ply_points():
    """X rows for the writer: 0, -0.0, 1e-5, 123456.7, 1234567, a denormal, NaN, +-inf"""
    vals = [0.0, -0.0, 1e-5, 123456.7, 1234567.0, 1e-45, float("nan"), float("inf"), float("-inf"), 0.1, -2.5, 1e10]
    X = np.array([[vals[i], vals[(i + 1) % len(vals)], vals[(i + 5) % len(vals)]] for i in range(len(vals))], np.float32)
    rgb = np.array([[(7 * i) % 256, (255 - i) % 256, (100 * i) % 256] for i in range(len(vals))], np.uint8)
    return X, rgb
