"""Host-side helpers on cloud dicts (numpy): order-preserving compaction, the 3 px dedup as the first-claim rule (whole:
np_dedup; in its phases: np_claim, np_keep) and bit-exact comparison — what the tests, tools/bench_filter_resident.py and tools/bench_dedup_resident.py compare the
device-resident filter and dedup stages with."""
import numpy as np

ARRAYS = ("X", "obs_off", "key", "obs_view", "obs_pl", "obs_seg", "obs_xy")


def np_compact(c, keep, X_new=None, min_obs=-1):
    """Order-preserving compaction of a host cloud dict (obs_off with its sentinel): the points with keep != 0 and more
    than min_obs observations (min_obs < 0: no count test)."""
    off = c["obs_off"].astype(np.int64)
    k = np.diff(off)
    sel = np.asarray(keep).astype(bool)
    if min_obs >= 0:
        sel = sel & (k > min_obs)
    osel = np.repeat(sel, k)
    X = (c["X"] if X_new is None else X_new)[sel]
    return {"n_points": int(sel.sum()), "n_obs": int(k[sel].sum()), "X": X,
            "obs_off": np.concatenate([[0], np.cumsum(k[sel])]).astype(np.uint64), "key": c["key"][sel],
            "obs_view": c["obs_view"][osel], "obs_pl": c["obs_pl"][osel], "obs_seg": c["obs_seg"][osel],
            "obs_xy": c["obs_xy"][osel]}


DEDUP_CELL = 3
UNCLAIMED = 0xFFFFFFFF


def dedup_claims(n_views, width, height):
    """An empty claim map for np_dedup: one entry per 3 px cell of every view (0xFFFFFFFF = no point has touched it)."""
    w, h = int(np.ceil(np.float32(width) / np.float32(DEDUP_CELL))), int(np.ceil(np.float32(height) / np.float32(DEDUP_CELL)))
    return np.full((int(n_views), h, w), UNCLAIMED, np.uint32)


def _cells_and_owners(c, claims, index_base):
    """(cell per valid observation, run-wide point index per valid observation, n_points) of a host cloud dict on the
    grid of `claims`: the cell rule of eg3d_host_filter_close_2d."""
    off = np.asarray(c["obs_off"]).astype(np.int64)
    n = len(off) - 1
    V, h, w = claims.shape
    if index_base + n >= UNCLAIMED:
        raise ValueError("index_base + n_points must stay below 2^32 - 1")
    a, b = int(off[0]), int(off[-1])
    view = np.asarray(c["obs_view"], np.int32)[a:b].astype(np.int64)
    xy = np.asarray(c["obs_xy"], np.float32).reshape(-1, 2)[a:b]
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = xy[:, 0] / np.float32(DEDUP_CELL), xy[:, 1] / np.float32(DEDUP_CELL)   # float32, a true division
        ok = (view >= 0) & (view < V) & (fx > -1) & (fy > -1) & (fx < np.float32(w)) & (fy < np.float32(h))  # NaN fails
        cx, cy = np.trunc(np.where(ok, fx, 0)).astype(np.int64), np.trunc(np.where(ok, fy, 0)).astype(np.int64)
    ok &= (cx >= 0) & (cy >= 0) & (cx < w) & (cy < h)     # (-1, 0) truncates to cell 0
    owner = np.repeat(np.arange(n, dtype=np.int64), np.diff(off)) + int(index_base)
    return ((view * h + cy) * w + cx)[ok], owner[ok], n


def np_claim(c, claims, index_base=0):
    """The claim pass alone (eg3d_dedup_claim, eg3d_host_dedup_claim): claims[cell] = min(claims[cell], index_base + i)
    over the observations of every point i, in place. Clouds may be claimed in any order; maps are joined with
    np.minimum(a, b, out=a). Returns claims."""
    cell, owner, _ = _cells_and_owners(c, claims, index_base)
    np.minimum.at(claims.reshape(-1), cell, owner.astype(np.uint32))
    return claims


def np_keep(c, claims, index_base=0):
    """The keep pass alone (eg3d_dedup_keep, eg3d_host_dedup_keep) against the map as it stands: the uint8 mask with
    keep[i] = some observation of i lies in a cell that holds index_base + i."""
    cell, owner, n = _cells_and_owners(c, claims, index_base)
    keep = np.zeros(n, np.uint8)
    mine = claims.reshape(-1)[cell] == owner
    keep[owner[mine] - int(index_base)] = 1
    return keep


def np_dedup(c, n_views, width, height, claims=None, index_base=0):
    """The 3 px dedup (eg3d_host_filter_close_2d, eg3d_dedup_device) of a host cloud dict as the first-claim rule: the first
    point that touches a cell is always kept, so keep[i] = some observation of i lies in a valid cell whose smallest
    touching point index is i. Two order-independent passes: a minimum per cell, one test per point. claims: a map from
    dedup_claims that is updated in place (None: a fresh one); with the map of cloud A and index_base = |A| the mask of
    cloud B is the second half of the mask of A || B. Returns the uint8 mask."""
    if claims is None:
        claims = dedup_claims(n_views, width, height)
    return np_keep(c, np_claim(c, claims, index_base), index_base)


def same_cloud(a, b):
    """None when the two cloud dicts are identical bit for bit (all seven arrays, in order), else what differs."""
    if int(a["n_points"]) != int(b["n_points"]) or int(a["n_obs"]) != int(b["n_obs"]):
        return "counts %d/%d vs %d/%d" % (a["n_points"], a["n_obs"], b["n_points"], b["n_obs"])
    for name in ARRAYS:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        if name == "obs_off":
            x, y = x.astype(np.uint64), y.astype(np.uint64)
        if x.shape != y.shape or x.dtype.itemsize != y.dtype.itemsize or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            return name
    return None
