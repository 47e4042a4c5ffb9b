"""Host-side helpers on cloud dicts (numpy): order-preserving compaction and bit-exact comparison — what the tests and
tools/bench_filter_resident.py compare the device-resident filter stage with."""
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
