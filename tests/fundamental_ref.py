"""An independent restatement of the fundamental-matrix estimator (eg3d_host_estimate_fundamental on the host,
eg3d_estimate_fundamental on the device), in Python integers and NumPy. It takes nothing from edgegraph3d_amd and is written
from the description of the algorithm, by other numerical routes than csrc/eg3d_fund_core.h on purpose:

  stream          SplitMix64 in Python integers; one stream per ordered pair, started at stream_seed(rng_seed, i * V + j)
  sample          8 distinct indices, next() % n each, a duplicate is drawn again
  common points   dictionaries per view: the last observation of a view id wins, ids outside [0, V) are ignored, ascending id
  fit             Hartley normalisation in np.longdouble; the null vector by an SVD of the n x 9 design matrix (the native
                  code takes the eigenvector of the 9 x 9 normal matrix, which squares the condition number); rank 2 by
                  zeroing the smallest singular value of the 3 x 3; F = T2' Fn T1 in np.longdouble; scaled by 1 / F33, or
                  to unit Frobenius norm when |F33| <= 1e-12 * norm
  residual        the larger of the two squared point-to-line distances, 1e300 when it is not finite
  selection       median = sorted[n // 2]; the smallest median wins, the earlier iteration on a tie (strict <)
  inliers, refit  residual <= max(sigma^2, 1e-12), sigma = 2.5 * 1.4826 * (1 + 5 / (n - 8)) * sqrt(best median); with at
                  least 8 inliers the fit over them replaces the winner if its median is <= the best

Next to the matrix every pair gets a REPORT (winning iteration, best median, inlier count, whether the refit ran and was kept,
the scaling branch) and the relative MARGINS of its decisions. A pair is DECIDED when every margin is at least DELTA: only
then has the estimator one answer that does not depend on the last bits of a residual, and only then is the native result
compared with this one."""
import numpy as np

LD = np.longdouble
MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MIN_COMMON = 10
SAMPLE = 8
DEFAULT_ITERATIONS = 300
HUGE = 1e300

# max|F - F_ref| / max|F_ref| per ordered pair: 100 times the worst value of the host statement against this file over all
# cases of tests/fundamental_cases.py that are compared (the hand-made ones, Synth(0), Synth(2)), measured on a CPU
# (x86-64, 80-bit long double):
#   worst 4.83e-12, case "synth0" (Synth(0), rng_seed 0), ordered pair (0, 2), 18 common points
# The factor 100 allows for the conditioning of other samples (the normal-equations route squares the condition number).
# The device needs no allowance of its own: it returns the host statement's bits.
TOL = 4.83e-10
# the smallest relative margin a decision must have: pixel coordinates near 1e3 amplify a change of F into a residual by ~1e4
DELTA = 1e4 * TOL


# ---- the stream -------------------------------------------------------------------------------------------------------------
class SplitMix64:
    def __init__(self, seed):
        self.s = seed & MASK

    def next(self):
        self.s = (self.s + GOLDEN) & MASK
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        return z ^ (z >> 31)

    def below(self, n):
        return self.next() % n


def stream_seed(rng_seed, ij):
    return (rng_seed & MASK) ^ ((GOLDEN * (ij + 1)) & MASK)


def draw_sample(rng, n):
    """8 distinct indices below n (n >= 8): a duplicate is drawn again"""
    idx = []
    while len(idx) < SAMPLE:
        c = rng.below(n)
        if c not in idx:
            idx.append(c)
    return idx


# ---- common points ----------------------------------------------------------------------------------------------------------
def observations(V, seeds):
    """per view {point id: (x, y)}: the last observation with that view id; ids outside [0, V) are ignored"""
    off, view, xy = seeds
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    per_view = [dict() for _ in range(V)]
    for p in range(len(off) - 1):
        for k in range(int(off[p]), int(off[p + 1])):
            v = int(view[k])
            if 0 <= v < V:
                per_view[v][p] = (xy[k, 0], xy[k, 1])
    return per_view


def correspondences(per_view, i, j):
    """x1, y1 (on view i), x2, y2 (on view j) of the points seen from both, ascending point id"""
    ids = sorted(per_view[i].keys() & per_view[j].keys())
    a = np.array([per_view[i][p] for p in ids], np.float64).reshape(-1, 2)
    b = np.array([per_view[j][p] for p in ids], np.float64).reshape(-1, 2)
    return a[:, 0], a[:, 1], b[:, 0], b[:, 1]


# ---- the fit ----------------------------------------------------------------------------------------------------------------
def _hartley(x, y):
    """(..., n) coordinates -> normalised coordinates and T (..., 3, 3): centroid to the origin, mean distance sqrt(2)"""
    x, y = x.astype(LD), y.astype(LD)
    cx, cy = x.mean(-1, keepdims=True), y.mean(-1, keepdims=True)
    d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2).mean(-1, keepdims=True)
    s = np.where(d > 1e-12, np.sqrt(LD(2)) / np.where(d > 1e-12, d, 1), LD(1))
    T = np.zeros(x.shape[:-1] + (3, 3), LD)
    T[..., 0, 0] = T[..., 1, 1] = s[..., 0]
    T[..., 0, 2] = -(s * cx)[..., 0]
    T[..., 1, 2] = -(s * cy)[..., 0]
    T[..., 2, 2] = 1
    return (x - cx) * s, (y - cy) * s, T


def fit(x1, y1, x2, y2):
    """The normalised 8-point fit of x2' F x1 = 0 over the last axis (n >= 8) of float64 arrays of any leading shape.
    Returns F (..., 3, 3), ok (...) (False: a degenerate fit, F is zero) and frob (...) (True: scaled to unit Frobenius norm,
    False: to F33 = 1)."""
    x1, y1, x2, y2 = (np.asarray(a, np.float64) for a in (x1, y1, x2, y2))
    finite = np.isfinite(x1 + y1 + x2 + y2).all(-1)
    # a fit with a non-finite coordinate is degenerate; the SVD must not see it, so it gets finite stand-ins (k, k^2, k^3, k^4)
    stand_in = np.arange(x1.shape[-1], dtype=np.float64)
    x1, y1, x2, y2 = (np.where(finite[..., None], a, stand_in ** (e + 1)) for e, a in enumerate((x1, y1, x2, y2)))
    u1, v1, T1 = _hartley(x1, y1)
    u2, v2, T2 = _hartley(x2, y2)
    one = np.ones_like(u1)
    design = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, one], -1).astype(np.float64)
    Fn = np.linalg.svd(design, full_matrices=True)[2][..., -1, :].reshape(design.shape[:-2] + (3, 3))
    U, S, Vt = np.linalg.svd(Fn)
    S[..., 2] = 0
    Fn = (U * S[..., None, :]) @ Vt
    F = (np.swapaxes(T2, -1, -2) @ Fn.astype(LD) @ T1).astype(np.float64)
    with np.errstate(all="ignore"):
        nrm = np.sqrt((F * F).sum((-1, -2)))
        ok = finite & np.isfinite(nrm) & (nrm > 0)
        f33 = F[..., 2, 2]
        frob = ~(np.abs(f33) > 1e-12 * nrm)
        scale = np.where(frob, 1.0 / nrm, 1.0 / f33)
        F = np.where(ok[..., None, None], F * scale[..., None, None], 0.0)
    return F, ok, frob


def residuals(F, x1, y1, x2, y2):
    """(..., 3, 3) matrices, (n,) coordinates -> (..., n): the larger squared distance of a point from the epipolar line of
    its partner, of the two images; 1e300 where that is not finite"""
    h1 = np.stack([x1, y1, np.ones_like(x1)], -1)
    h2 = np.stack([x2, y2, np.ones_like(x2)], -1)
    with np.errstate(all="ignore"):
        l2 = np.einsum("...ab,nb->...na", F, h1)   # F x1: the line in image 2
        l1 = np.einsum("...ba,nb->...na", F, h2)   # F' x2: the line in image 1
        d2 = (l2 * h2).sum(-1) ** 2 / (l2[..., 0] ** 2 + l2[..., 1] ** 2)
        d1 = (l1 * h1).sum(-1) ** 2 / (l1[..., 0] ** 2 + l1[..., 1] ** 2)
        d = np.maximum(d1, d2)
    return np.where(np.isfinite(d), d, HUGE)


def median(res):
    return np.sort(res, -1)[..., res.shape[-1] // 2]


def inlier_threshold(best_med, n):
    sigma = 2.5 * 1.4826 * (1.0 + 5.0 / (n - SAMPLE + (1 if n == SAMPLE else 0))) * np.sqrt(best_med)
    return max(sigma * sigma, 1e-12)


def _rel(a, b):
    """the distance of a from b relative to b (b > 0); infinite when there is no a"""
    return abs(a - b) / b if b > 0 else (0.0 if a == b else np.inf)


def lmeds(x1, y1, x2, y2, iterations, seed):
    """One ordered pair. Returns (F (3, 3) or None, report). The margins of the report:
      gap      from the best median up to the smallest median of an iteration that drew another SET of points (the same set
               in another order gives the same matrix up to rounding: which of the two wins does not matter)
      thr_gap  from the inlier threshold to the nearest residual of the winner
      mgap     from the best median to the refit's (infinite where no refit ran)"""
    n = len(x1)
    rng = SplitMix64(seed)
    idx = np.array([draw_sample(rng, n) for _ in range(iterations)], np.int64)
    Fs, ok, frob = fit(x1[idx], y1[idx], x2[idx], y2[idx])
    med = np.where(ok, median(residuals(Fs, x1, y1, x2, y2)), HUGE)
    report = {"n": n, "n_degenerate": int((~ok).sum()), "n_nondegenerate": int(ok.sum()), "it": -1, "best_med": HUGE, "n_in": 0,
              "refit_ran": False, "refit_kept": False, "frobenius": False, "gap": np.inf, "thr_gap": np.inf, "mgap": np.inf}
    best_it, best = -1, HUGE
    for it in range(iterations):  # strict <: the earlier iteration keeps a tie; a median of 1e300 never wins
        if med[it] < best:
            best_it, best = it, float(med[it])
    if best_it < 0:
        return None, report
    F, is_frob = Fs[best_it], bool(frob[best_it])
    others = [float(med[it]) for it in range(iterations) if set(idx[it]) != set(idx[best_it])]
    report.update(it=best_it, best_med=best, gap=_rel(min(others), best) if others else np.inf)
    res = residuals(F, x1, y1, x2, y2)
    thr = inlier_threshold(best, n)
    inl = np.nonzero(res <= thr)[0]
    report.update(n_in=len(inl), thr=thr, thr_gap=float(np.min(np.abs(res - thr)) / thr))
    if len(inl) >= SAMPLE:
        Fr, ok_r, frob_r = fit(x1[inl], y1[inl], x2[inl], y2[inl])
        report["refit_ran"] = True
        if ok_r:
            med_r = float(median(residuals(Fr, x1, y1, x2, y2)))
            report["mgap"] = _rel(med_r, best)
            if med_r <= best:
                F, is_frob = Fr, bool(frob_r)
                report["refit_kept"] = True
    report["frobenius"] = is_frob
    return F, report


def decided(report, delta=DELTA):
    return min(report["gap"], report["thr_gap"], report["mgap"]) >= delta


def estimate(V, seeds, iterations=0, rng_seed=0):
    """All ordered pairs: F [V, V, 9], valid [V, V] u8, n_common [V, V] u32, {"n_pairs_valid", "n_pairs_failed"} and the
    reports {(i, j): report} of the pairs with at least 10 common points."""
    iterations = iterations or DEFAULT_ITERATIONS
    per_view = observations(V, seeds)
    F = np.zeros((V, V, 9))
    valid = np.zeros((V, V), np.uint8)
    ncom = np.zeros((V, V), np.uint32)
    reports = {}
    for i in range(V):
        for j in range(V):
            if i == j or not per_view[i] or not per_view[j]:
                continue
            x1, y1, x2, y2 = correspondences(per_view, i, j)
            ncom[i, j] = len(x1)
            if len(x1) < MIN_COMMON:
                continue
            Fij, reports[(i, j)] = lmeds(x1, y1, x2, y2, iterations, stream_seed(rng_seed, i * V + j))
            if Fij is not None:
                F[i, j] = Fij.reshape(9)
                valid[i, j] = 1
    st = {"n_pairs_valid": int(valid.sum()), "n_pairs_failed": len(reports) - int(valid.sum())}
    return F, valid, ncom, st, reports


def distance(F, F_ref):
    """max|F - F_ref| / max|F_ref| of one pair"""
    return float(np.max(np.abs(np.asarray(F) - F_ref)) / np.max(np.abs(F_ref)))
