"""Request windows for the lane-group Gauss-Newton solver (coop_gn_groups, eg3d_dev_coopgn.h), shared by its GPU test
(tests/test_gpu_coop_gn.py: probe against oracle, bit for bit) and the CPU pin of the oracle's solves against scipy
(tests/test_dlt_forms.py). A window holds up to 32 requests (request j on lane j, None = a lane with want = false); a
request is the Gauss-Newton solve of em_add_new_observation_to_3Dpositions: rows (view, x, y) that project a true point
plus noise, the last one optionally passed as the extra (ADD) observation, and a float start point. Every window is built
to hit an edge of the solver: row counts around the packing and group boundaries, the packing rule, long requests of
different lengths in one round, and a spread of convergence (stops at iteration 2-3, far starts, never converging,
rejected results, singular normal equations, starts on or behind a camera plane, NaN)."""
import numpy as np

from edgegraph3d_amd import host

ROWS = (2, 3, 4, 5, 6, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 1000)
ROWS_LONG_ONLY = (4096,)  # only on the variants with the long-request path (a small build refuses it anyway)
PACK_MAX = 32  # EG3D_GN_PACK_MAX
REQ = 32  # EG3D_COOP_REQ


def cams_mid_range(cam_P):
    """The product's rule (eg3d_api.hip, DevScene::cams_mid_range): every non-zero entry of the first three rows of every
    camera in 2^-100 .. 2^100 (NaN fails)."""
    p = np.asarray(cam_P, np.float32).reshape(-1, 16)[:, :12]
    a = np.abs(p[p != 0])
    return int(bool(np.all((a >= np.float32(7.888609052210118e-31)) & (a <= np.float32(1.2676506002282294e+30)))))


class Rig:
    def __init__(self, name, cam_P, Xs):
        self.name = name
        self.P = np.ascontiguousarray(np.asarray(cam_P, np.float32).reshape(-1, 16))
        self.M = self.P.reshape(-1, 4, 4)[:, :3, :].astype(np.float64)
        self.V = len(self.P)
        self.mid = cams_mid_range(self.P)
        self.Xs = Xs  # true points of the scene (float64, in front of the cameras)
        # camera centres: M[:, :, :3] C = -M[:, :, 3]
        self.C = np.stack([np.linalg.solve(m[:, :3], -m[:, 3]) for m in self.M])

    def project(self, v, X):
        h = self.M[v] @ np.append(X, 1.0)
        return h[:2] / h[2]


def rigs():
    """c5: the 16-view rig of BASELINE config 5; wide: a 256-view rig of the C4 generator; tiny: the c5 rig with camera
    entries outside 2^-100 .. 2^100 (half the views scaled by 2^-104 — the same projections, rows outside the shared-
    reciprocal regime —, the others with one entry of 1e-33), so the product's rule gives cams_mid_range = 0."""
    s5 = host.Synth(5)
    P5 = s5.scene_np()["cam_P"].reshape(-1, 16).copy()
    X5, _, _, _ = s5.points(400)
    cw = host.default_config(4)
    cw.n_views, cw.n_seeds, cw.n_curves = 256, 10, 20
    sw = host.Synth(cw)
    Pw = sw.scene_np()["cam_P"].reshape(-1, 16).copy()
    Xw, _, _, _ = sw.points(400)
    Pt = P5.copy()
    Pt[0::2] *= np.float32(2.0 ** -104)
    Pt[1::2, 9] = np.float32(1e-33)
    out = [Rig("c5", P5, X5.astype(np.float64)), Rig("wide", Pw, Xw.astype(np.float64)), Rig("tiny", Pt, X5.astype(np.float64))]
    assert out[0].mid == 1 and out[1].mid == 1 and out[2].mid == 0
    return out


KINDS = ("near", "far", "edge9", "wild", "nonconv", "singular", "plane", "behind", "nan_obs", "nan_x0")


def make_request(rig, n, kind, rng, has_extra=True):
    """One request of n rows on `rig`. Returns dict(view [n] int32, xy [n, 2] float32, X0 [3] float32, has_extra, kind)."""
    Xt = rig.Xs[rng.integers(len(rig.Xs))]
    k_views = min(n, rig.V)
    views = rng.choice(rig.V, k_views, replace=False)
    if n > k_views:  # more rows than views: views repeat (the solver does not care)
        views = np.concatenate([views, rng.integers(0, rig.V, n - k_views)])
    if kind == "singular":  # every row from one view: rank-2 normal equations
        views = np.full(n, views[0])
    views = views.astype(np.int32)
    sigma = {"near": 0.5, "far": 0.5, "edge9": rng.uniform(2.6, 3.4), "wild": 0.5, "nonconv": 0.5, "singular": 0.5,
             "plane": 0.5, "behind": 0.5, "nan_obs": 0.5, "nan_x0": 0.5}[kind]
    xy = np.array([rig.project(v, Xt) for v in views]) + rng.normal(0, sigma, (n, 2))
    if kind == "wild":  # observations of no single point: uniform over the image
        xy = rng.uniform(0, 1600, (n, 2))
    X0 = Xt + rng.normal(0, 0.02, 3)
    if kind in ("far", "edge9"):
        X0 = Xt + rng.normal(0, 25.0, 3)
    elif kind == "wild":
        X0 = Xt + rng.normal(0, 60.0, 3)
    elif kind == "nonconv":
        # start far beyond the rig, rows with very different noise: Gauss-Newton keeps moving for all 30 iterations
        X0 = Xt + rng.normal(0, 1.0, 3) * 4000.0
        xy = xy + rng.normal(0, 40.0, (n, 2)) * (rng.uniform(size=(n, 1)) < 0.3)
    elif kind == "plane":  # start on the principal plane of one of the request's views: zH ~ 0
        v = int(views[rng.integers(n)])
        m = rig.M[v]
        u = rng.normal(size=3)
        z = m[2] @ np.append(Xt, 1.0)
        X0 = Xt - z / (m[2, :3] @ u) * u
    elif kind == "behind":  # start behind one of the request's cameras
        v = int(views[rng.integers(n)])
        X0 = rig.C[v] + (rig.C[v] - Xt) * rng.uniform(0.05, 0.5)
    xy = xy.astype(np.float32)
    X0 = X0.astype(np.float32)
    if kind == "nan_obs":
        xy[rng.integers(n), rng.integers(2)] = np.nan
    elif kind == "nan_x0":
        X0[rng.integers(3)] = np.nan
    return dict(view=views, xy=xy, X0=X0, has_extra=bool(has_extra), kind=kind)


class Windows:
    """Named windows on one rig, flattened into the probe's tables (tests/probe/eg3d_probe.h eg3d_probe_coop_gn) and the
    oracle's request list (oracle/binding.py gn_add_batch)."""

    def __init__(self, rig):
        self.rig = rig
        self.names, self.wins = [], []

    def add(self, name, reqs):
        assert len(reqs) <= REQ and any(r is not None for r in reqs)
        self.names.append(name)
        self.wins.append(list(reqs) + [None] * (REQ - len(reqs)))

    def tables(self):
        nw = len(self.wins)
        req_i = np.zeros((nw * REQ, 5), np.int32)
        req_f = np.zeros((nw * REQ, 5), np.float32)
        ov, oxy, roff = [], [], [0]
        rv, rxy = [], []
        n_req = np.zeros(nw * REQ, np.int32)
        at = 0
        for w, win in enumerate(self.wins):
            for j, r in enumerate(win):
                e = w * REQ + j
                if r is None:
                    continue
                n = len(r["view"])
                nb = n - 1 if r["has_extra"] else n
                req_i[e] = (1, at, nb, 1 if r["has_extra"] else 0, r["view"][-1] if r["has_extra"] else 0)
                req_f[e, 0:2] = r["xy"][-1] if r["has_extra"] else 0
                req_f[e, 2:5] = r["X0"]
                ov.append(r["view"][:nb])
                oxy.append(r["xy"][:nb])
                at += nb
                rv.append(r["view"])
                rxy.append(r["xy"])
                roff.append(roff[-1] + n)
                n_req[e] = n
        return dict(req_i=req_i, req_f=req_f, obs_view=np.ascontiguousarray(np.concatenate(ov), np.int32),
                    obs_xy=np.ascontiguousarray(np.concatenate(oxy), np.float32), n_req=n_req,
                    row_off=np.array(roff, np.uint32), row_view=np.concatenate(rv).astype(np.int32),
                    row_xy=np.concatenate(rxy).astype(np.float32),
                    X0=np.array([r["X0"] for win in self.wins for r in win if r is not None], np.float32))

    def kinds(self):
        return [r["kind"] for win in self.wins for r in win if r is not None]


def add_bulk(W, rig, rng, n_windows):
    """Random windows: 1..32 requests, 2..32 rows (15 % of them 33..300), lanes left empty now and then, starts near and
    far, noise on both sides of the acceptance threshold, inconsistent rows. Numbers are what let one rounding difference in
    the double accumulators show through the float result; these windows give the comparison thousands of solves."""
    kinds = np.array(("near", "far", "edge9", "nonconv", "wild"))
    n_req = rng.integers(1, REQ + 1, n_windows)
    R = int(n_req.sum())
    sizes = np.where(rng.uniform(size=R) < 0.15, rng.integers(33, 301, R), rng.integers(2, PACK_MAX + 1, R))
    kind = kinds[rng.integers(0, len(kinds), R)]
    pid = np.repeat(np.arange(R), sizes)
    view = rng.integers(0, rig.V, len(pid)).astype(np.int32)
    Xt = rig.Xs[rng.integers(0, len(rig.Xs), R)]
    h = np.einsum("nij,nj->ni", rig.M[view], np.concatenate([Xt[pid], np.ones((len(pid), 1))], 1))
    sigma = np.select([kind == "edge9", kind == "nonconv"], [rng.uniform(2.6, 3.4, R), 40.0 * (rng.uniform(size=R) < 0.5)], 0.5)
    xy = h[:, :2] / h[:, 2:3] + rng.normal(0, 1, (len(pid), 2)) * sigma[pid][:, None]
    wild = kind[pid] == "wild"
    xy[wild] = rng.uniform(0, 1600, (int(wild.sum()), 2))
    spread = np.select([kind == "near", kind == "nonconv", kind == "wild"], [0.02, 4000.0, 60.0], 25.0)
    X0 = (Xt + rng.normal(0, 1, (R, 3)) * spread[:, None]).astype(np.float32)
    xy = xy.astype(np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)])
    extra = rng.uniform(size=R) < 0.8
    r = 0
    for w in range(n_windows):
        reqs = []
        for _ in range(n_req[w]):
            a, b = off[r], off[r + 1]
            reqs.append(dict(view=view[a:b], xy=xy[a:b], X0=X0[r], has_extra=bool(extra[r]), kind=str(kind[r])))
            r += 1
        if n_req[w] > 2 and rng.uniform() < 0.3:  # an empty lane inside the window
            reqs[int(rng.integers(0, n_req[w] - 1))] = None
        W.add("bulk_%d" % w, reqs)


def build_windows(rig, seed, long_rows=True, n_bulk=0):
    """The windows of one rig (see the module docstring). long_rows=False leaves out the 4096-row requests."""
    rng = np.random.default_rng(seed)
    W = Windows(rig)
    mk = lambda n, kind, ex=True: make_request(rig, n, kind, rng, ex)
    rows = ROWS + (ROWS_LONG_ONLY if long_rows else ())
    # every row count alone on lane 0 (how the central solves call it), with and without the extra observation
    for n in rows:
        for kind in ("near", "far"):
            W.add("single_%d_%s" % (n, kind), [mk(n, kind, ex=(n % 2 == 0))])
    # every short size 2..32 (G = the row count), packed with a convergence spread
    spread = ("near", "near", "far", "edge9", "nonconv", "wild")
    for n in range(2, PACK_MAX + 1):
        k = max(1, min(REQ, 64 // n))
        W.add("pack_%dx%d" % (k, n), [mk(n, spread[(i + n) % len(spread)]) for i in range(k)])
    # 32 requests of 2 rows: 64 rows, 32 groups, the most the per-group sums hold — every kind
    for rep in range(2):
        W.add("pack_32x2_%d" % rep, [mk(2, KINDS[(i + rep) % len(KINDS)]) for i in range(REQ)])
    # sizes that break the contiguity rule: a round stops at the first request that does not fit
    for sizes in ((30, 30, 5, 2), (20, 20, 30, 4, 3), (32, 31, 2, 2, 32), (3, 32, 30, 2, 29, 5), (16, 16, 16, 17, 15, 2)):
        W.add("contig_" + "_".join(map(str, sizes)), [mk(n, spread[i % len(spread)]) for i, n in enumerate(sizes)])
    # want = false lanes between active ones
    for gaps in range(3):
        reqs = [None] * REQ
        for j in range(gaps, REQ, 3 + gaps):
            reqs[j] = mk(int(rng.choice((2, 3, 5, 7, 9, 33, 65))), spread[j % len(spread)])
        W.add("gaps_%d" % gaps, reqs)
    # short and long requests in one window, lanes interleaved
    W.add("mixed_short_long", [mk(n, spread[i % len(spread)]) for i, n in enumerate((5, 40, 3, 100, 2, 33, 31, 64, 7, 65))])
    W.add("mixed_short_long_2", [mk(n, spread[i % len(spread)]) for i, n in enumerate((2, 129, 6, 32, 33, 4, 200, 8))])
    # long requests of different lengths in one round: groups run out of rows before cmax
    W.add("long_lengths", [mk(n, spread[i % len(spread)]) for i, n in enumerate((33, 200, 64, 129, 65, 127, 128, 63))])
    W.add("long_lengths_2", [mk(n, spread[i % len(spread)]) for i, n in enumerate((1000, 33, 34, 500))])
    # more long requests than one round takes (per_round = 64 >> lg): 32 of 33 rows (G = 2), 20 of 65..129, 12 of 200..400
    W.add("long_32x33", [mk(33, spread[i % len(spread)]) for i in range(REQ)])
    W.add("long_20", [mk(int(rng.integers(65, 130)), spread[i % len(spread)]) for i in range(20)])
    W.add("long_12", [mk(int(rng.integers(200, 401)), spread[i % len(spread)]) for i in range(12)])
    # two long requests: groups of 32 lanes (one round) — with short ones around them
    W.add("long_pair_200_180", [mk(200, "near"), mk(180, "far")])
    W.add("long_pair_1000_65", [mk(3, "near"), mk(1000, "far"), mk(65, "edge9"), mk(4, "far")])
    W.add("long_pair_129_100", [None, mk(129, "nonconv"), None, mk(100, "near")])
    W.add("long_6x1000", [mk(1000, spread[i % len(spread)]) for i in range(6)])
    # the convergence spread inside one window, at short, packed-long and long sizes
    for n in (3, 6, 8, 31, 33, 65, 200):
        k = min(REQ, max(1, 64 // n)) if n <= PACK_MAX else min(len(KINDS), 8)
        W.add("kinds_%d" % n, [mk(n, KINDS[i % len(KINDS)]) for i in range(max(k, min(REQ, len(KINDS))))])
    if n_bulk:
        add_bulk(W, rig, rng, n_bulk)
    return W
