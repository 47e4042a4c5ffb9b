#!/usr/bin/env python3
"""K18, cloud-to-cloud nearest distances on resident clouds (include/eg3d/nearest.hpp), against the route a caller has
without it: fetch_device_output + host.cloud_nearest on the host's threads (OMP_NUM_THREADS; 16 where the numbers of
DESIGN.md 4 "K18" were taken). One GPU. One JSON line on stdout and profiles/nearest.json (EG3D_BENCH_OUT overrides the
path). No figure here is a pass condition, and no ratio is promised: the file is where the numbers go.

Per workload one child process under its own time limit (a fault or a hang of one workload ends that child, and nothing is
started after it):
  c2, c3    the cloud match_refpoints(device_only=True) leaves resident for host.Synth(2) / Synth(3) (C2, C3')
  synth     --synth-points points on random polylines in the unit cube, uploaded (a C4-sized cloud is 56 000 000)
The reference cloud is the cloud itself jittered by a normal deviate of 0.2 max_dist per axis, the same size, resident as
a bare array; max_dist = cell = --max-dist-fraction of the cloud's largest extent. Both directions — accuracy (cloud against
an index over the reference) and completeness (reference against an index over the cloud) — are timed: the index build and
the query, each as the wall time of the call with a synchronised host clock and as the call's own event time. The device
route and the host route ALTERNATE within one loop of `reps` repetitions after the warm-ups; medians with minimum and
maximum are reported. With --mappings the query is also timed with 1, 8 and 64 lanes per query (EG3D_K18_GROUP, read when
an index is built), alternating. Every device figure is compared with the host statement's before its time is reported.

  python tools/bench_nearest.py [reps=5] [--workloads c2,c3,synth] [--synth-points N] [--max-dist-fraction 0.01] [--mappings]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser(description="K18 against fetch + the host statement")
ap.add_argument("reps", nargs="?", type=int, default=5)
ap.add_argument("--workloads", default="c2,c3,synth")
ap.add_argument("--synth-points", type=int, default=56000000)
ap.add_argument("--max-dist-fraction", type=float, default=0.01)
ap.add_argument("--mappings", action="store_true")
ap.add_argument("--limit", type=int, default=420, help="time limit of one workload's child process, seconds")
ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
opt = ap.parse_args()
reps = max(3, opt.reps)
WARMUPS = 1
F = np.float32
EXACT = ("n_queries", "n_dropped", "n_nonfinite", "n_within", "sum_q32", "n_below")


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def synth_cloud(n, rng):
    """points along random straight polylines of 200 points each in the unit cube: spatially coherent, as a chain cloud is"""
    m = (n + 199) // 200
    a, b = rng.uniform(0, 1, (m, 1, 3)), rng.normal(0, 0.05, (m, 1, 3))
    t = np.linspace(0, 1, 200, dtype=np.float64).reshape(1, 200, 1)
    return (a + t * b).reshape(-1, 3)[:n].astype(F)


def worker(wl):
    from edgegraph3d_amd import api, host
    rng = np.random.default_rng(18)
    if wl == "synth":
        s = host.Synth(0)
        ctx = api.Context(s.scene)
        X = synth_cloud(opt.synth_points, rng)
        Xd = ctx.upload(X)
        cloud = api.points_cloud(Xd, len(X))
        fetch = lambda: Xd.numpy(F, (len(X), 3))        # (a bare array: the copy is X alone)
    else:
        s = host.Synth({"c2": 2, "c3": 3}[wl])
        ctx = api.Context(s.scene)
        ctx.match_refpoints(s.seeds, device_only=True)
        cloud = ctx.last_device_output()
        fetch = lambda: ctx.fetch_device_output()["X"]  # (what a caller has today: the whole cloud comes back)
        X = fetch()
    n = len(X)
    finite = np.isfinite(X).all(axis=1)
    md = float(F(opt.max_dist_fraction * float(np.ptp(X[finite], axis=0).max())))
    ref = (X + rng.normal(0, 0.2 * md, X.shape)).astype(F)
    Rd = ctx.upload(ref)
    ref_cloud = api.points_cloud(Rd, n)
    th = (md, 0.5 * md, 0.25 * md)
    d2d, nnd = ctx.device_alloc(4 * n), ctx.device_alloc(4 * n)
    t = {k: [] for k in ("build_ref_wall", "build_ref_ev", "acc_wall", "acc_ev", "build_own_wall", "build_own_ev", "comp_wall", "comp_ev",
                         "fetch", "host_acc", "host_comp")}
    dev_fig = host_fig = ix_stats = None
    for i in range(WARMUPS + reps):
        w0 = time.perf_counter()
        ix_ref = ctx.cloud_index(cloud=ref_cloud, cell=md)
        w1 = time.perf_counter()
        acc = ctx.nearest_device(ix_ref, md, cloud=cloud, thresholds=th, to_host=False, d2=d2d, nn=nnd)["stats"]
        w2 = time.perf_counter()
        ix_own = ctx.cloud_index(cloud=cloud, cell=md)
        w3 = time.perf_counter()
        comp = ctx.nearest_device(ix_own, md, cloud=ref_cloud, thresholds=th, to_host=False, d2=d2d, nn=nnd)["stats"]
        w4 = time.perf_counter()
        ix_stats = (ix_ref.stats, ix_own.stats)
        ix_ref.close()
        ix_own.close()
        Xh = fetch()
        w5 = time.perf_counter()
        hacc = host.cloud_nearest(ref, Xh, md, thresholds=th)[2]
        w6 = time.perf_counter()
        hcomp = host.cloud_nearest(Xh, ref, md, thresholds=th)[2]
        w7 = time.perf_counter()
        dev_fig, host_fig = (acc, comp), (hacc, hcomp)
        if i >= WARMUPS:
            for k, v in (("build_ref_wall", w1 - w0), ("acc_wall", w2 - w1), ("build_own_wall", w3 - w2), ("comp_wall", w4 - w3),
                         ("fetch", w5 - w4), ("host_acc", w6 - w5), ("host_comp", w7 - w6)):
                t[k].append(v * 1e3)
            t["build_ref_ev"].append(ix_stats[0]["ms_build"])
            t["build_own_ev"].append(ix_stats[1]["ms_build"])
            t["acc_ev"].append(acc["ms_kernel"])
            t["comp_ev"].append(comp["ms_kernel"])
    same = all(d[k] == h[k] for d, h in zip(dev_fig, host_fig) for k in EXACT) and all(
        F(d[k]).view(np.uint32) == F(h[k]).view(np.uint32) for d, h in zip(dev_fig, host_fig) for k in ("min_d2", "max_d2", "median_d2"))
    m = {k: stats(v) for k, v in t.items()}
    device_ms = sum(m[k]["median"] for k in ("build_ref_wall", "acc_wall", "build_own_wall", "comp_wall"))
    host_ms = sum(m[k]["median"] for k in ("fetch", "host_acc", "host_comp"))
    out = {"points": n, "max_dist": md, "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0")),
           "index_ref": {k: ix_stats[0][k] for k in ("n_indexed", "n_cells", "max_cell_points", "dims")},
           "index_own": {k: ix_stats[1][k] for k in ("n_indexed", "n_cells", "max_cell_points", "dims")},
           "accuracy": {k: dev_fig[0][k] for k in ("n_within", "mean", "median", "n_below")},
           "completeness": {k: dev_fig[1][k] for k in ("n_within", "mean", "median", "n_below")},
           "ms": m, "device_both_directions_ms": device_ms, "host_route_ms": host_ms, "host_route_over_device": host_ms / device_ms,
           "same_figures_as_host_statement": bool(same),
           # what the query kernel must move at the least: the queries read (12 B), d2 and nn written (8 B), per direction; what it
           # reads of the index depends on the data (the runs of up to 16 rows per query) and is served from L2 for coherent queries
           "query_bytes_min": 20 * n, "build_bytes_min": (12 + 16 + 12) * n}
    if opt.mappings:
        maps = {}
        idx = {}
        for g in ("1", "8", "64"):
            os.environ["EG3D_K18_GROUP"] = g
            idx[g] = ctx.cloud_index(cloud=ref_cloud, cell=md)
        os.environ.pop("EG3D_K18_GROUP", None)
        ev = {g: [] for g in idx}
        for i in range(WARMUPS + reps):
            for g in idx:       # alternating
                st = ctx.nearest_device(idx[g], md, cloud=cloud, thresholds=th, to_host=False, d2=d2d, nn=nnd)["stats"]
                assert all(st[k] == dev_fig[0][k] for k in EXACT), g
                if i >= WARMUPS:
                    ev[g].append(st["ms_kernel"])
        for g in idx:
            maps[g] = stats(ev[g])
            idx[g].close()
        out["accuracy_query_ms_by_lanes_per_query"] = maps
    ctx.close()
    s.close()
    print("RESULT " + json.dumps(out), flush=True)


if opt.worker:
    worker(opt.worker)
    sys.exit(0)

line = {"reps": reps, "warmups": WARMUPS}
for wl in [w for w in opt.workloads.split(",") if w]:
    cmd = ["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), str(reps), "--worker", wl, "--max-dist-fraction",
           str(opt.max_dist_fraction), "--synth-points", str(opt.synth_points)] + (["--mappings"] if opt.mappings else [])
    p = subprocess.run(cmd, capture_output=True, text=True)
    got = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not got:
        # a fault, an abort or the time limit: nothing more is started on this GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        line[wl] = {"error": "the %s child ended with status %d" % (wl, p.returncode)}
        print(json.dumps(line))
        sys.exit(1)
    line[wl] = json.loads(got[0][len("RESULT "):])
    print("%s done" % wl, file=sys.stderr, flush=True)
print(json.dumps(line))
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "nearest.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
