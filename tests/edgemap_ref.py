"""The edge maps of the source images, restated in numpy from the rules E1 - E7 of include/eg3d/host_edgemap.hh (not from
the C++): whole-array integer arithmetic in int64, the borders by index arrays, the hysteresis by
scipy.ndimage.label with a 3 x 3 structure — a labelling of the candidates, so no propagation order exists in it."""
import numpy as np
from scipy import ndimage

MAX_DIM, MAX_PASSES, MAX_THRESHOLD = 16384, 4, 65535
BINOMIAL = (1, 4, 6, 4, 1)


def reflect101(i, n):
    """E2's fold of an index array."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.abs(i) % p
    return np.where(i >= n, p - i, i)


def grey(rgb):
    c = np.asarray(rgb, np.uint8).astype(np.int64)
    return (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14


def smooth(y):
    h, w = y.shape
    cols = [reflect101(np.arange(w) + k - 2, w) for k in range(5)]
    rows = [reflect101(np.arange(h) + k - 2, h) for k in range(5)]
    hs = sum(BINOMIAL[k] * y[:, cols[k]] for k in range(5))
    vs = sum(BINOMIAL[k] * hs[rows[k], :] for k in range(5))
    return (vs + 128) >> 8


def shifted(a, dr, dc, fill=None):
    """b[r][c] = a[r + dr][c + dc]; outside the image: `fill`, or the nearest border pixel when fill is None."""
    h, w = a.shape
    if fill is None:
        r = np.clip(np.arange(h) + dr, 0, h - 1)
        c = np.clip(np.arange(w) + dc, 0, w - 1)
        return a[np.ix_(r, c)]
    out = np.full((h + 2, w + 2), fill, a.dtype)
    out[1:-1, 1:-1] = a
    return out[1 + dr:1 + dr + h, 1 + dc:1 + dc + w]


def gradient(y):
    p = lambda dr, dc: shifted(y, dr, dc)
    gx = (p(-1, 1) + 2 * p(0, 1) + p(1, 1)) - (p(-1, -1) + 2 * p(0, -1) + p(1, -1))
    gy = (p(1, -1) + 2 * p(1, 0) + p(1, 1)) - (p(-1, -1) + 2 * p(-1, 0) + p(-1, 1))
    return gx, gy


def classes(rgb, low, high, smooth_passes=1, l2=False):
    """(candidate, strong) boolean arrays of one image: E1 - E5 and the first half of E6."""
    y = grey(rgb)
    for _ in range(smooth_passes):
        y = smooth(y)
    gx, gy = gradient(y)
    if l2:
        m, lo, hi = gx * gx + gy * gy, low * low, high * high
    else:
        m, lo, hi = np.abs(gx) + np.abs(gy), low, high
    n = lambda dr, dc: shifted(m, dr, dc, fill=0)
    x, yy = np.abs(gx), np.abs(gy) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    horizontal = yy < t22
    vertical = ~horizontal & (yy > t67)
    s_neg = (gx ^ gy) < 0
    keep_h = (m > n(0, -1)) & (m >= n(0, 1))
    keep_v = (m > n(-1, 0)) & (m >= n(1, 0))
    keep_pos = (m > n(-1, -1)) & (m > n(1, 1))      # s = 1
    keep_neg = (m > n(-1, 1)) & (m > n(1, -1))      # s = -1
    kept = np.where(horizontal, keep_h, np.where(vertical, keep_v, np.where(s_neg, keep_neg, keep_pos)))
    candidate = kept & (m > lo)
    return candidate, candidate & (m > hi)


def edge_map(rgb, low, high, smooth_passes=1, l2=False):
    """(mask uint8 [H, W], n_candidates, n_strong) of one image."""
    candidate, strong = classes(rgb, low, high, smooth_passes, l2)
    labels, _ = ndimage.label(candidate, structure=np.ones((3, 3), int))
    good = np.unique(labels[strong])
    mask = np.isin(labels, good[good > 0]) & candidate
    return mask.astype(np.uint8), int(candidate.sum()), int(strong.sum())


def edge_maps(images, low, high, smooth_passes=1, l2=False):
    """As host.edge_maps: (masks, the four counts)."""
    if not len(images) or not (0 <= low <= high <= MAX_THRESHOLD) or not (0 <= smooth_passes <= MAX_PASSES):
        raise ValueError("refused by E7")
    masks, nc, ns, npx = [], 0, 0, 0
    for im in images:
        m, c, s = edge_map(im, low, high, smooth_passes, l2)
        masks.append(m)
        nc, ns, npx = nc + c, ns + s, npx + m.size
    return masks, {"n_views": len(images), "n_pixels": npx, "n_candidates": nc, "n_strong": ns, "n_edges": int(sum(int(m.sum()) for m in masks))}
