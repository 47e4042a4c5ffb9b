"""The case table of the edge maps (K19): every case a name, its images and its parameters; all arrays seeded. What the
numpy restatement (tests/edgemap_ref.py) gives for a case is computed once (expected) and shared by the host and the GPU
tests. The cases that exist to break a propagation scheme assert here, with the restatement alone, that they are what
they claim to be."""
import functools
import os
from collections import deque

import numpy as np
from scipy import ndimage

import edgemap_ref as R
import png_util

TILE = 32   # K19_TILE of csrc/eg3d_k19_edgemap.h (tests/test_edgemap_host.py holds the two together)
EIGHT = np.ones((3, 3), int)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dtu006_edges", "0000.png")


def rgb_of(grey):
    return np.repeat(np.asarray(grey, np.uint8)[:, :, None], 3, 2)


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def step(kind, h=37, w=40, lo=90, hi=150):
    yy, xx = np.mgrid[0:h, 0:w]
    bright = {"vertical": xx >= w // 2, "horizontal": yy >= h // 2, "diagonal": xx > yy, "antidiagonal": xx + yy > w - 1}[kind]
    return rgb_of(np.where(bright, hi, lo))


def scene(seed=7, h=35, w=67, amplitude=6):
    """A disc and a rectangle on a ramp, each channel with its own gain, under seeded noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    g = 60.0 + 0.4 * xx + 0.3 * yy
    g[(xx - 0.3 * w) ** 2 + (yy - 0.5 * h) ** 2 < (0.3 * h) ** 2] += 70
    g[int(0.2 * h):int(0.75 * h), int(0.6 * w):int(0.9 * w)] -= 35
    rgb = np.stack([g * 1.0, g * 0.8 + 20, 200 - g * 0.5], -1) + rng.integers(-amplitude, amplitude + 1, (h, w, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8)


def _bench():
    """tools/bench_edgemaps.py: the synthetic photographs and the serpentine are the benchmark's, used here at test sizes"""
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import bench_edgemaps
    finally:
        sys.path.remove(tools)
    return bench_edgemaps


# ---- the serpentine: the outline of a band that winds through the whole image, cut open next to its only strong pixel --------
SERPENTINE = dict(_bench().SERPENTINE_PARAMS)


def serpentine(w=130, h=66):
    return _bench().serpentine_view(w, h)


def _check_serpentine(im):
    cand, strong = R.classes(im, **SERPENTINE)
    mask = R.edge_map(im, **SERPENTINE)[0]
    h, w = cand.shape
    assert ndimage.label(cand, structure=EIGHT)[1] == 1 and strong.sum() == 1
    degree = ndimage.convolve(cand.astype(int), EIGHT, mode="constant") - 1
    assert degree[cand].max() <= 3 and (degree[cand] == 1).sum() == 2          # a 1 pixel wide path with two ends
    assert not ndimage.binary_erosion(cand, structure=np.ones((2, 2))).any()    # no 2 x 2 block
    tiles = {(y // TILE, x // TILE) for y, x in np.argwhere(cand)}
    assert tiles == {(ty, tx) for ty in range(-(-h // TILE)) for tx in range(-(-w // TILE))}      # every tile, the partial ones too
    # breadth first from the strong pixel: it sits at one end, the other end is far, and the walk crosses tile borders in
    # all four directions
    start = tuple(np.argwhere(strong)[0])
    dist, queue, moves = {start: 0}, deque([start]), set()
    while queue:
        y, x = queue.popleft()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                q = (y + dy, x + dx)
                if 0 <= q[0] < h and 0 <= q[1] < w and cand[q] and q not in dist:
                    dist[q] = dist[(y, x)] + 1
                    moves.add((q[0] // TILE - y // TILE, q[1] // TILE - x // TILE))
                    queue.append(q)
    ends = [tuple(p) for p in np.argwhere(cand & (degree == 1))]
    assert min(dist[e] for e in ends) <= 2 and max(dist.values()) > 1000
    assert {(1, 0), (-1, 0), (0, 1), (0, -1)} <= moves
    assert np.array_equal(mask, cand.astype(np.uint8))                          # the restatement keeps the whole serpentine


# ---- one outline whose two parts meet only diagonally, across the corner the tiles (0,0), (0,1), (1,0) and (1,1) share ------------
CORNER = dict(low=30, high=60, smooth_passes=0, l2=False)


def corner():
    g = np.full((64, 64), 100, np.int32)
    g[TILE:54, 10:TILE + 1] = 110          # its top edge ends at (31, 31), its right edge starts at (32, 32)
    g[51:56, 18:23] = 105                  # the outline cut open at the bottom
    g[TILE, 20] += 12                      # strong pixels on the top edge
    return rgb_of(g)


def _check_corner(im):
    cand, strong = R.classes(im, **CORNER)
    a, b = TILE - 1, TILE
    assert cand[a, a] and cand[b, b] and not cand[a, b] and not cand[b, a]
    assert ndimage.label(cand, structure=EIGHT)[1] == 1 and strong.any()
    without = cand.copy()
    without[a, a] = False
    labels, n = ndimage.label(without, structure=EIGHT)
    assert n == 2 and len(np.unique(labels[strong])) == 1 and labels[b, b] not in labels[strong]
    assert np.array_equal(R.edge_map(im, **CORNER)[0], cand.astype(np.uint8))


def weak_only():
    g = np.full((40, 45), 100, np.int32)
    g[8:30, 9:33] = 110
    return rgb_of(g)


def golden_crop(w=256, h=192):
    """A crop of a dtu006 edge map, x 255, blurred into a grey picture: dense real structure."""
    m = png_util.read_png_edge_mask(GOLDEN)
    ys, xs = np.nonzero(m)
    y0 = int(min(max(np.median(ys) - h // 2, 0), m.shape[0] - h))
    x0 = int(min(max(np.median(xs) - w // 2, 0), m.shape[1] - w))
    g = ndimage.uniform_filter(m[y0:y0 + h, x0:x0 + w].astype(np.float64) * 255.0, 3, mode="nearest")
    return np.stack([g, 0.5 * g + 40, 255 - g], -1).round().astype(np.uint8)


def _case(name, images, low, high, smooth_passes=1, l2=False):
    return dict(name=name, images=[np.ascontiguousarray(i) for i in images], low=low, high=high, smooth_passes=smooth_passes, l2=l2)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for k, (w, h) in enumerate(((1, 1), (1, 7), (7, 1), (2, 2), (3, 3))):
        for passes in (0, 1, 4):
            out.append(_case("size_%dx%d_p%d" % (w, h, passes), [noise(100 + k, h, w)], 10, 200, passes))
    out.append(_case("constant", [np.full((20, 23, 3), 137, np.uint8)], 0, 0))
    for kind in ("vertical", "horizontal", "diagonal", "antidiagonal"):
        out.append(_case("step_" + kind, [step(kind)], 20, 60))
    for passes in (0, 1, 4):
        for l2 in (False, True):
            out.append(_case("scene_p%d_%s" % (passes, "l2" if l2 else "l1"), [scene()], 40, 120, passes, l2))
    out.append(_case("scene_low_equals_high", [scene()], 80, 80))
    out.append(_case("scene_zero_bounds", [scene()], 0, 0))
    out.append(_case("noise_widest_bounds", [noise(5, 33, 65)], 0, 65535, 0, True))
    s, c = serpentine(), corner()
    _check_serpentine(s)
    _check_corner(c)
    out.append(_case("serpentine", [s], **SERPENTINE))
    out.append(_case("diagonal_across_tile_corner", [c], **CORNER))
    out.append(_case("weak_only", [weak_only()], 30, 100, 0))
    out.append(_case("three_views", [scene(11), noise(12, 7, 1), step("diagonal", 70, 33)], 40, 120))
    out.append(_case("golden_crop", [golden_crop()], 60, 180))
    out.append(_case("golden_crop_l2_p0", [golden_crop()], 60, 180, 0, True))
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def names():
    return [c["name"] for c in cases()]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def params(c):
    return dict(low=c["low"], high=c["high"], smooth_passes=c["smooth_passes"], l2=c["l2"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """(masks, counts) of the restatement for the case; computed once, never changed."""
    c = case(name)
    masks, counts = R.edge_maps(c["images"], **params(c))
    for m in masks:
        m.setflags(write=False)
    return masks, counts


COUNTS = ("n_views", "n_pixels", "n_candidates", "n_strong", "n_edges")
# two small views put around a case's images when it runs as part of a larger call
FILLERS = (noise(900, 9, 45), scene(901, 33, 31))


def full_view(seed=0, w=1600, h=1200):
    """one of the benchmark's synthetic photographs at full size"""
    return _bench().synthetic_view(w, h, seed)
