#!/usr/bin/env python3
"""K19, the edge maps of the source images on the device (include/eg3d/edgemap.hh), against their host statement on the
host's threads (OMP_NUM_THREADS; 16 where the numbers of DESIGN_LOG.md were taken), and the polyline graphs of the result.
One GPU. One JSON line on stdout and profiles/edgemaps.json (EG3D_BENCH_OUT overrides the path). No figure here is a pass
condition, and no ratio is promised: the file is where the numbers go.

The workload: --views (25) synthetic photographs of --size (1600x1200) — rendered discs, ellipse outlines and rectangles
on a ramp, each channel with its own gain, under seeded noise (synthetic_view). The device call and the host call
ALTERNATE within one loop of `reps` repetitions after the warm-up; every stage is reported as median, minimum and
maximum: the wall time of the call with a host clock, and the stages the call itself reports (device: upload, front-end
kernels, hysteresis and masks, copy back, from events; host: classes and hysteresis, wall). The device masks and counts are
compared with the host statement's before any time is reported. Then host.plg_views_from_masks on the masks, and the worst
input of the hysteresis — one view whose only strong pixel ends a path through every tile (serpentine_view) — on both.

  python tools/bench_edgemaps.py [reps=5] [--views 25] [--size 1600x1200] [--low 40] [--high 100]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUPS = 1


def synthetic_view(width, height, seed):
    """A seeded RGB picture [height, width, 3] uint8 with curved and straight contours of several contrasts."""
    rng = np.random.default_rng(1900 + seed)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
    g = 70.0 + 40.0 * xx / width + 25.0 * yy / height
    s = min(width, height)
    for _ in range(6):      # discs
        cx, cy, r = rng.uniform(0, width), rng.uniform(0, height), rng.uniform(0.04, 0.18) * s
        g[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] += rng.choice([-1, 1]) * rng.uniform(15, 70)
    for _ in range(6):      # ellipse outlines, a few pixels wide
        cx, cy = rng.uniform(0, width), rng.uniform(0, height)
        a, b = rng.uniform(0.05, 0.3) * s, rng.uniform(0.05, 0.3) * s
        d = np.sqrt(((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2)
        g[np.abs(d - 1.0) < 3.0 / min(a, b)] += rng.uniform(20, 60)
    for _ in range(8):      # rectangles
        x0, y0 = int(rng.uniform(0, 0.9) * width), int(rng.uniform(0, 0.9) * height)
        x1, y1 = x0 + int(rng.uniform(0.03, 0.3) * width), y0 + int(rng.uniform(0.03, 0.3) * height)
        g[y0:y1, x0:x1] += rng.choice([-1, 1]) * rng.uniform(10, 60)
    rgb = np.stack([g, 0.8 * g + 25.0, 210.0 - 0.6 * g], -1) + rng.integers(-5, 6, (height, width, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8)


# what serpentine_view is made for: with these parameters its candidates are one 1 pixel wide path and one of them is strong
SERPENTINE_PARAMS = dict(low=30, high=60, smooth_passes=0, l2=True)


def serpentine_view(width, height):
    """A grey picture whose candidates under SERPENTINE_PARAMS are the outline of a band that winds through the whole image
    in horizontal bars, 12 rows apart — cut open beside its only strong pixel, (2, 14), so that every other candidate is
    reached from there along the whole outline. Needs width >= 40, height >= 30."""
    g = np.full((height, width), 100, np.int32)
    rows = list(range(3, height - 15, 12)) + [height - 5]   # the last bar's lower edge lies in the last row but one
    x0, x1 = 2, width - 1
    for k, r in enumerate(rows):
        g[r:r + 4, x0:x1] = 110
        if k + 1 < len(rows):
            g[r + 4:rows[k + 1], (x1 - 4 if k % 2 == 0 else x0):(x1 if k % 2 == 0 else x0 + 4)] = 110
    g[1:6, 8:13] = 105      # the cut: a contrast of 5 on either side gives no candidate
    g[3, 14] += 12          # the strong pixel above it
    return np.repeat(g.astype(np.uint8)[:, :, None], 3, 2)


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed_pair(api, host, images, params, reps):
    """The device call and the host call alternating; returns (device times, host times, device stats, masks)."""
    dev = {k: [] for k in ("wall", "ms_upload", "ms_kernel", "ms_hysteresis", "ms_copy")}
    hst = {k: [] for k in ("wall", "ms_kernel", "ms_hysteresis")}
    masks = stats = None
    for i in range(WARMUPS + reps):
        t0 = time.perf_counter()
        masks, stats = api.edge_maps(images, **params)
        t1 = time.perf_counter()
        hmasks, hstats = host.edge_maps(images, **params)
        t2 = time.perf_counter()
        assert all(np.array_equal(a, b) for a, b in zip(masks, hmasks)), "the device masks differ from the host statement's"
        assert all(stats[k] == hstats[k] for k in ("n_views", "n_pixels", "n_candidates", "n_strong", "n_edges")), (stats, hstats)
        if i >= WARMUPS:
            dev["wall"].append((t1 - t0) * 1e3)
            hst["wall"].append((t2 - t1) * 1e3)
            for k in dev:
                if k != "wall":
                    dev[k].append(stats[k])
            for k in hst:
                if k != "wall":
                    hst[k].append(hstats[k])
    return {k: spread(v) for k, v in dev.items()}, {k: spread(v) for k, v in hst.items()}, stats, masks


def main():
    ap = argparse.ArgumentParser(description="K19 against the host statement")
    ap.add_argument("reps", nargs="?", type=int, default=5)
    ap.add_argument("--views", type=int, default=25)
    ap.add_argument("--size", default="1600x1200")
    ap.add_argument("--low", type=int, default=40)
    ap.add_argument("--high", type=int, default=100)
    opt = ap.parse_args()
    reps = max(3, opt.reps)
    width, height = (int(v) for v in opt.size.split("x"))
    sys.path.insert(0, ROOT)
    from edgegraph3d_amd import api, host
    images = [synthetic_view(width, height, v) for v in range(opt.views)]
    params = dict(low=opt.low, high=opt.high, smooth_passes=1, l2=False)
    line = {"reps": reps, "warmups": WARMUPS, "views": opt.views, "width": width, "height": height, "params": params,
            "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0"))}
    dev, hst, stats, masks = timed_pair(api, host, images, params, reps)
    counts = ("n_pixels", "n_candidates", "n_strong", "n_edges", "hysteresis_rounds")
    line["photographs"] = {"device_ms": dev, "host_ms": hst, "counts": {k: stats[k] for k in counts},
                           "host_wall_over_device_wall": hst["wall"]["median"] / dev["wall"]["median"],
                           # what must cross the host's link at the least: the images up, one byte a pixel back
                           "link_bytes": 4 * stats["n_pixels"]}
    t = []
    n_polylines = 0
    for i in range(WARMUPS + reps):
        t0 = time.perf_counter()
        graphs = host.plg_views_from_masks(masks)
        if i >= WARMUPS:
            t.append((time.perf_counter() - t0) * 1e3)
        n_polylines = sum(int(g["n_polylines"]) for g in graphs)
    line["plg_views_from_masks"] = {"ms": spread(t), "n_polylines": n_polylines}
    dev, hst, stats, _ = timed_pair(api, host, [serpentine_view(width, height)], SERPENTINE_PARAMS, 3)
    line["worst_hysteresis_one_view"] = {"device_ms": dev, "host_ms": hst, "counts": {k: stats[k] for k in counts}}
    print(json.dumps(line))
    out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "edgemaps.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
