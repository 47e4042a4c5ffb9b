#!/usr/bin/env python3
"""K14, the FP64 triangulation of caller-supplied tracks (include/eg3d_triangulate.h), against its host statement
(eg3d_host_triangulate on 16 threads) on one GPU. One JSON line on stdout and profiles/triangulate.json (EG3D_BENCH_OUT
overrides the path). No figure here is a pass condition, and no speed-up is promised: the file is where the numbers go.

Per workload one child process under its own time limit (a fault or a hang of one workload ends that child, and nothing is
started after it):
  c2, c3   Synth(2) / Synth(3) (C2, C3'):
             seeds   the seed tracks through eg3d_triangulate in both modes (EG3D_TRI_REFINE starts from the seeds' true
                     points): the call's wall time, its ms_stage / ms_kernel / ms_copy, batches;
             cloud   match_refpoints(device_only=True), then eg3d_triangulate_device(NULL, EG3D_TRI_REFINE) on the
                     resident cloud: wall time and ms_stage / ms_kernel;
           and the host statement on the same arrays (the cloud's from a host copy), 16 threads.
  c4long   a C4-shaped cloud with long lists: the 256-view rig of the C4 generator, `--long-tracks` tracks of 75
           observations each (C4's points carry ~75), uploaded once and run through eg3d_triangulate_device in both
           modes, and a second time with the staging budget at a sixteenth of the observations (the batched path).
Every GPU result is compared with the host statement's, byte for byte, before its time is reported. There is one form of
the kernel (lane groups): the one-lane form for short tracks is not built, so there is no short / long split to report.

  python tools/bench_triangulate.py [reps=5] [--workloads c2,c3,c4long] [--long-tracks N] [--limit SECONDS]
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

ap = argparse.ArgumentParser(description="K14 against the host statement")
ap.add_argument("reps", nargs="?", type=int, default=5)
ap.add_argument("--workloads", default="c2,c3,c4long")
ap.add_argument("--long-tracks", type=int, default=50000)
ap.add_argument("--limit", type=int, default=300, help="time limit of one workload's child process, seconds")
ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
opt = ap.parse_args()
reps = max(3, opt.reps)
HOST_THREADS = 16


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(fn):
    """reps + 1 runs, the first dropped: (wall ms of each, the last result)."""
    ms, out = [], None
    for i in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        if i:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, out


def host_leg(host, P, rows, off, view, xy, X0, mode):
    ms, out = timed(lambda: host.triangulate(P, off, view, xy, X0=X0 if mode == 1 else None, mode=mode, dlt_rows=rows,
                                             n_threads=HOST_THREADS))
    return ms, out


def report(n, m, gpu_ms, st_all, host_ms, same):
    g, h = stats(gpu_ms), stats(host_ms)
    r = {"tracks": int(n), "observations": int(m), "call_ms": g, "host_statement_16_threads_ms": h,
         "tracks_per_s": n / (g["median"] * 1e-3), "host_tracks_per_s": n / (h["median"] * 1e-3),
         "host_over_call": h["median"] / g["median"], "same_bytes_as_host_statement": bool(same)}
    for k in ("ms_stage", "ms_kernel", "ms_copy"):
        r[k] = stats([s[k] for s in st_all])
    for k in ("n_batches", "n_valid", "n_short", "n_degenerate"):
        r[k] = int(st_all[-1][k])
    return r


def same_rows(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def worker(wl):
    from edgegraph3d_amd import _cdefs as D
    from edgegraph3d_amd import api, host
    rows = api.lib().eg3d_dlt_rows()
    r = {}
    if wl in ("c2", "c3"):
        s = host.Synth({"c2": 2, "c3": 3}[wl])
        P = s.scene_np()["cam_P"]
        ctx = api.Context(s.scene)
        off, view, xy = s.seeds_np()
        X0 = s.seed_truth().astype(np.float32)
        for mode, name in ((0, "seeds_from_scratch"), (1, "seeds_refine")):
            st_all = []

            def call():
                X, v, f, st = ctx.triangulate(off, view, xy, X0=X0 if mode == 1 else None, mode=mode)
                st_all.append(st)
                return X, v, f
            gpu_ms, got = timed(call)
            host_ms, want = host_leg(host, P, rows, off, view, xy, X0, mode)
            r[name] = report(len(off) - 1, off[-1], gpu_ms, st_all[1:], host_ms, same_rows(got, want))
        ctx.match_refpoints(s.seeds, device_only=True)
        cloud = ctx.fetch_device_output()
        n = cloud["n_points"]
        Xd, vd, fd = ctx.device_alloc(12 * n), ctx.device_alloc(n), ctx.device_alloc(n)
        st_all = []

        def call_dev():
            st_all.append(ctx.triangulate_device(None, 1, X_out=Xd, valid=vd, flags=fd)[3])
        gpu_ms, _ = timed(call_dev)
        got = (Xd.numpy(np.float32, (n, 3)), vd.numpy(np.uint8), fd.numpy(np.uint8))
        coff = cloud["obs_off"].astype(np.uint32)
        host_ms, want = host_leg(host, P, rows, coff, cloud["obs_view"], cloud["obs_xy"], cloud["X"], 1)
        r["cloud_refine"] = report(n, cloud["n_obs"], gpu_ms, st_all[1:], host_ms, same_rows(got, want))
        ctx.close()
    else:
        cw = host.default_config(4)
        cw.n_views, cw.n_seeds, cw.n_curves = 256, 10, 20
        s = host.Synth(cw)
        P = s.scene_np()["cam_P"].reshape(-1, 16)
        ctx = api.Context(s.scene)
        rng = np.random.default_rng(14)
        n, k, V = opt.long_tracks, 75, len(P)
        Xs = s.points(400)[0].astype(np.float64)
        Xt = Xs[rng.integers(0, len(Xs), n)]
        view = np.argsort(rng.random((n, V)), axis=1)[:, :k].astype(np.int32).reshape(-1)   # 75 distinct views per track
        M = P.reshape(-1, 4, 4)[:, :3, :].astype(np.float64)
        h = np.einsum("nij,nj->ni", M[view], np.repeat(np.concatenate([Xt, np.ones((n, 1))], 1), k, axis=0))
        xy = (h[:, :2] / h[:, 2:3] + rng.normal(0, 0.5, (n * k, 2))).astype(np.float32)
        X0 = (Xt + rng.normal(0, 0.05, (n, 3))).astype(np.float32)
        off = (np.arange(n + 1, dtype=np.uint64) * k)
        keep = [ctx.upload(X0), ctx.upload(off[:-1]), ctx.upload(view), ctx.upload(xy)]
        dev = D.DeviceEdgePoints()
        dev.n_points, dev.n_obs, dev.complete = n, n * k, 1
        dev.X, dev.obs_off, dev.obs_view, dev.obs_xy = (a.ptr for a in keep)
        Xd, vd, fd = ctx.device_alloc(12 * n), ctx.device_alloc(n), ctx.device_alloc(n)
        off32 = off.astype(np.uint32)
        for mode, name in ((0, "from_scratch"), (1, "refine")):
            host_ms, want = host_leg(host, P, rows, off32, view, xy, X0, mode)
            for budget, tag in ((None, ""), (max(k, n * k // 16), "_sixteen_batches")):
                if budget is None:
                    os.environ.pop("EG3D_TRI_STAGE_OBS", None)
                else:
                    os.environ["EG3D_TRI_STAGE_OBS"] = str(budget)
                st_all = []

                def call_dev():
                    st_all.append(ctx.triangulate_device(dev, mode, X_out=Xd, valid=vd, flags=fd)[3])
                gpu_ms, _ = timed(call_dev)
                got = (Xd.numpy(np.float32, (n, 3)), vd.numpy(np.uint8), fd.numpy(np.uint8))
                r[name + tag] = report(n, n * k, gpu_ms, st_all[1:], host_ms, same_rows(got, want))
                if budget is not None:
                    r[name + tag]["stage_budget_observations"] = int(budget)
        os.environ.pop("EG3D_TRI_STAGE_OBS", None)
        ctx.close()
    s.close()
    print("RESULT " + json.dumps(r), flush=True)


if opt.worker:
    worker(opt.worker)
    sys.exit(0)

line = {"reps": reps, "host_threads": HOST_THREADS, "kernel_forms": "lane groups only (the one-lane form is not built: no short / long split)"}
for wl in [w for w in opt.workloads.split(",") if w]:
    cmd = ["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), str(reps), "--worker", wl,
           "--long-tracks", str(opt.long_tracks)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    got = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not got:
        # a fault, an abort or the time limit: nothing more is started on this GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        line[wl] = {"error": "the %s child ended with status %d" % (wl, p.returncode)}
        print(json.dumps(line))
        sys.exit(1)
    line[wl] = json.loads(got[0][len("RESULT "):])
print(json.dumps(line))
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "triangulate.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
