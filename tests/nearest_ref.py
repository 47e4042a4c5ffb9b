"""An independent restatement of include/eg3d/host_nearest.hpp in numpy: brute force, FP32 elementwise, no grid. For every
query the squared distances to ALL reference points that may be indexed, the strict within rule, the smallest d2 and the
smallest index that attains it; then the figures by a sort and an integer sum. Nothing here is shared with the library."""
import numpy as np

INF_BITS = 0x7F800000
NONE = 0xFFFFFFFF


def _usable(X, keep):
    X = np.asarray(X, np.float32).reshape(-1, 3)
    kept = np.ones(len(X), bool) if keep is None else (np.asarray(keep).reshape(-1) != 0)
    finite = np.isfinite(X).all(axis=1)
    return X, kept, finite


def nearest(ref_X, X, max_dist, ref_keep=None, keep=None, thresholds=()):
    """(d2 [n] float32, nn [n] uint32, figures dict) of the definition."""
    R, rkept, rfin = _usable(ref_X, ref_keep)
    Q, qkept, qfin = _usable(X, keep)
    md = np.float32(max_dist)
    md2 = np.float32(md * md)
    ridx = np.nonzero(rkept & rfin)[0]
    Ru = R[ridx]
    n = len(Q)
    d2 = np.full(n, np.inf, np.float32)
    nn = np.full(n, NONE, np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in np.nonzero(qkept & qfin)[0]:
            if not len(Ru):
                break
            dx = (Q[i, 0] - Ru[:, 0]).astype(np.float32)
            dy = (Q[i, 1] - Ru[:, 1]).astype(np.float32)
            dz = (Q[i, 2] - Ru[:, 2]).astype(np.float32)
            d = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
            d = (d + (dz * dz).astype(np.float32)).astype(np.float32)
            ok = d < md2
            if ok.any():
                best = d[ok].min()
                d2[i] = best
                nn[i] = ridx[np.nonzero(ok & (d == best))[0][0]]   # (ridx ascends: the first is the smallest index)
    within = nn != NONE
    w = int(within.sum())
    bits = d2.view(np.uint32)
    t = np.asarray(thresholds, np.float32).reshape(-1)
    t2 = (t * t).astype(np.float32)
    fig = {"n_queries": n, "n_dropped": int((~qkept).sum()), "n_nonfinite": int((qkept & ~qfin).sum()), "n_within": w,
           "n_below": [int((d2[within] < v).sum()) for v in t2],
           "min_d2": np.float32(d2[within].min()) if w else np.float32(np.inf),
           "max_d2": np.float32(d2[within].max()) if w else np.float32(np.inf),
           "median_d2": np.sort(bits)[(w - 1) // 2].view(np.float32) if w else np.float32(np.inf),
           "sum_q32": int(sum(int(v) for v in (np.sqrt(d2[within].astype(np.float64)) * (4294967296.0 / np.float64(md))).astype(np.uint64)))}
    return d2, nn, fig


def index_figures(ref_X, cell, ref_keep=None):
    """n_dropped, n_nonfinite, n_indexed, origin, dims, n_cells and max_cell_points of the grid over ref_X, from the
    header's words: origin = the minimum, coordinate = floor((x - origin) / cell) in FP64."""
    R, kept, fin = _usable(ref_X, ref_keep)
    use = R[kept & fin]
    out = {"n_points": len(R), "n_dropped": int((~kept).sum()), "n_nonfinite": int((kept & ~fin).sum()), "n_indexed": len(use)}
    if not len(use):
        out.update(origin=np.zeros(3, np.float32), dims=[0, 0, 0], n_cells=0, max_cell_points=0)
        return out
    origin = use.min(axis=0)
    c = np.floor((use.astype(np.float64) - origin.astype(np.float64)) / np.float64(np.float32(cell))).astype(np.int64)
    _, counts = np.unique(c, axis=0, return_counts=True)
    out.update(origin=origin, dims=[int(v) + 1 for v in c.max(axis=0)], n_cells=len(counts), max_cell_points=int(counts.max()))
    return out
