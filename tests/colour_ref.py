"""An independent Python restatement of include/eg3d_colour.h and of the PLY writer of include/eg3d_host_colour.h, for the
CPU tests: numpy float32 scalars in the written order (a numpy float32 times a numpy float32 is a float32: no operation
here is done in double), np.rint for cvRound's ties-to-even, Python's int() for the truncation toward zero, and the LOOP
form of the border rule. No part of the library is used."""
import functools

import numpy as np

f32 = np.float32
ONE = f32(1.0)
LIMIT = f32(1e7)
MAX_OBS = 32767
FLAG_EMPTY = 1


@functools.lru_cache(maxsize=None)
def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101) as its documented loop."""
    if 0 <= p < n:
        return p
    if n == 1:
        return 0
    while True:
        p = -p if p < 0 else 2 * n - 2 - p
        if 0 <= p < n:
            return p


def coord_ok(v):
    v = f32(v)
    return bool(np.isfinite(v)) and bool(abs(v) < LIMIT)


def sample(img, px, py):
    """The three bytes of one observation; img [H, W, 3] uint8."""
    H, W = img.shape[:2]
    px, py = f32(px), f32(py)
    x, y = int(px), int(py)
    a, c = px - f32(x), py - f32(y)
    assert a.dtype == np.float32 and c.dtype == np.float32
    x0, x1, y0, y1 = reflect101(x, W), reflect101(x + 1, W), reflect101(y, H), reflect101(y + 1, H)
    out = []
    for ch in range(3):
        i00, i01, i10, i11 = f32(img[y0, x0, ch]), f32(img[y0, x1, ch]), f32(img[y1, x0, ch]), f32(img[y1, x1, ch])
        s = (i00 * (ONE - a) + i01 * a) * (ONE - c) + (i10 * (ONE - a) + i11 * a) * c
        assert s.dtype == np.float32
        out.append(int(np.rint(s)) & 0xff)
    return out


def colour(images, obs_off, obs_view, obs_xy, keep=None):
    """(refused, rgb [n, 3] uint8, flags [n] uint8, counts dict). Offsets must ascend over ALL points; the other checks
    apply to the points the mask keeps."""
    n = len(obs_off) - 1
    V = len(images)
    rgb, flags = np.zeros((n, 3), np.uint8), np.zeros(n, np.uint8)
    counts = {"n_coloured": 0, "n_empty": 0, "n_obs_sampled": 0}
    off = [int(o) for o in obs_off]
    if any(off[i + 1] < off[i] for i in range(n)):
        return True, None, None, None
    for i in range(n):
        if keep is not None and not keep[i]:
            continue
        a, b = off[i], off[i + 1]
        if b - a > MAX_OBS:
            return True, None, None, None
        sums = [0, 0, 0]
        for k in range(a, b):
            v, (px, py) = int(obs_view[k]), obs_xy[k]
            if not 0 <= v < V or images[v] is None or not coord_ok(px) or not coord_ok(py):
                return True, None, None, None
            for ch, byte in enumerate(sample(images[v], px, py)):
                sums[ch] += byte
        if b == a:
            flags[i] = FLAG_EMPTY
            counts["n_empty"] += 1
            continue
        rgb[i] = [s // (b - a) for s in sums]
        counts["n_coloured"] += 1
        counts["n_obs_sampled"] += b - a
    return False, rgb, flags, counts


def g_text(v):
    """`ostream << float`: %g of the widened value, precision 6."""
    return "%g" % float(f32(v))


def ply_bytes(X, rgb=None, keep=None):
    X = np.asarray(X, np.float32).reshape(-1, 3)
    n = len(X)
    kept = [i for i in range(n) if keep is None or keep[i]]
    head = ["ply", "format ascii 1.0", "element vertex %d" % len(kept), "property float x", "property float y", "property float z",
            "property uchar red", "property uchar green", "property uchar blue", "end_header"]
    text = "".join(l + "\n" for l in head)
    for i in kept:
        r, g, b = (255, 255, 255) if rgb is None else (int(c) for c in rgb[i])
        text += "%s %s %s %d %d %d" % (g_text(X[i, 0]), g_text(X[i, 1]), g_text(X[i, 2]), r, g, b)
        if i != n - 1:
            text += "\n"
    return text.encode()
