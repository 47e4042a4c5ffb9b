#!/usr/bin/env python3
"""K16, a 4 x 4 transform applied to a resident cloud's points (include/eg3d_transform.h), against the route a caller has
without it: copy the points to the host, transform them there on 16 threads, copy them back. One GPU. One JSON line on
stdout and profiles/transform.json (EG3D_BENCH_OUT overrides the path). No figure here is a pass condition, and no ratio
is promised: the file is where the numbers go.

Per workload one child process under its own time limit (a fault or a hang of one workload ends that child, and nothing is
started after it):
  c2, c3    the resident cloud of host.Synth(2) / Synth(3) (C2, C3') after match_refpoints(device_only=True)
  c4shape   a caller-built cloud of 56 000 000 seeded random points — the SIZE of C4's cloud (the 100 000-seed scaling
            workload), not its coordinates; the transform reads nothing but X, so only X is built (672 MB)
For each, medians of `reps` (10) repetitions after 2 warm-ups:
  device_out_of_place   eg3d_transform_device into a preallocated X_out: wall time of the call and the kernel's own time
  device_in_place       the same in place, with a pure rotation so that repeated calls do not drift in magnitude
  host_route            X device -> host, eg3d_host_transform_points on 16 threads, X host -> device: the three parts and
                        their sum. This is the LEAST that route can copy: a caller that fetches the whole cloud copies more.
The device result is compared with the host statement's, byte for byte, before its time is reported.

  python tools/bench_transform.py [reps=10] [--workloads c2,c3,c4shape] [--limit SECONDS]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser(description="K16 against the copy-transform-copy route")
ap.add_argument("reps", nargs="?", type=int, default=10)
ap.add_argument("--workloads", default="c2,c3,c4shape")
ap.add_argument("--limit", type=int, default=300, help="time limit of one workload's child process, seconds")
ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
opt = ap.parse_args()
reps = max(3, opt.reps)
WARMUPS = 2
HOST_THREADS = 16
C4_POINTS = 56_000_000


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(fn):
    """WARMUPS + reps runs, the warm-ups dropped: (wall ms of each, the last result)."""
    ms, out = [], None
    for i in range(WARMUPS + reps):
        t0 = time.perf_counter()
        out = fn()
        if i >= WARMUPS:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, out


def similarity():
    rng = np.random.default_rng(1600)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 2] = -Q[:, 2]
    T, Rot = np.eye(4), np.eye(4)
    T[:3, :3], T[:3, 3] = 2.5 * Q, [10.0, -20.0, 30.0]
    Rot[:3, :3] = Q
    return T, Rot


def worker(wl):
    from edgegraph3d_amd import _cdefs as D
    from edgegraph3d_amd import api, host
    hip = api._hip()
    T, Rot = similarity()
    keep_alive = []
    if wl == "c4shape":
        s = host.Synth(0)
        ctx = api.Context(s.scene)
        n = C4_POINTS
        X0 = np.random.default_rng(1601).standard_normal((n, 3), dtype=np.float32) * np.float32(100)
        keep_alive += [ctx.upload(X0), ctx.device_alloc(256)]   # the second block stands in for obs_off, which the call never reads
        dev = D.DeviceEdgePoints(n_points=n, n_obs=0, X=keep_alive[0].ptr, obs_off=keep_alive[1].ptr, complete=1)
    else:
        s = host.Synth({"c2": 2, "c3": 3}[wl])
        ctx = api.Context(s.scene)
        ctx.match_refpoints(s.seeds, device_only=True)
        dev = ctx.last_device_output()
        n = int(dev.n_points)
    x_ptr = C.cast(dev.X, C.c_void_p).value
    out = ctx.device_alloc(12 * n)
    host_X, back = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)

    def d2h():
        assert hip.hipMemcpy(host_X.ctypes.data, C.c_void_p(x_ptr), host_X.nbytes, 2) == 0
    d2h_ms, _ = timed(d2h)
    host_ms, _ = timed(lambda: host.transform_points(T, host_X, out=back))
    h2d_ms, _ = timed(lambda: hip.hipMemcpy(C.c_void_p(out.ptr), back.ctypes.data, back.nbytes, 1))
    st_out, st_in = [], []
    oop_ms, _ = timed(lambda: st_out.append(ctx.transform_device(T, out=out, cloud=dev)))
    same = out.numpy(np.float32, (n, 3)).tobytes() == back.tobytes()
    inp_ms, _ = timed(lambda: st_in.append(ctx.transform_device(Rot, cloud=dev)))
    a, b, c = stats(d2h_ms), stats(host_ms), stats(h2d_ms)
    g, gi = stats(oop_ms), stats(inp_ms)
    route = a["median"] + b["median"] + c["median"]
    r = {"points": n, "bytes_of_X": 12 * n,
         "device_out_of_place": {"call_ms": g, "ms_kernel": stats([x["ms_kernel"] for x in st_out[WARMUPS:]])},
         "device_in_place": {"call_ms": gi, "ms_kernel": stats([x["ms_kernel"] for x in st_in[WARMUPS:]])},
         "host_route": {"x_to_host_ms": a, "host_statement_ms": b, "x_to_device_ms": c, "sum_of_medians_ms": route,
                        "host_threads": HOST_THREADS},
         "host_route_over_device_call": route / g["median"], "n_nonfinite": int(st_out[-1]["n_nonfinite"]),
         "same_bytes_as_host_statement": bool(same)}
    ctx.close()
    s.close()
    print("RESULT " + json.dumps(r), flush=True)


if opt.worker:
    worker(opt.worker)
    sys.exit(0)

line = {"reps": reps, "warmups": WARMUPS, "host_threads": HOST_THREADS}
env = dict(os.environ, OMP_NUM_THREADS=str(HOST_THREADS))
for wl in [w for w in opt.workloads.split(",") if w]:
    cmd = ["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), str(reps), "--worker", wl]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env)
    got = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not got:
        # a fault, an abort or the time limit: nothing more is started on this GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        line[wl] = {"error": "the %s child ended with status %d" % (wl, p.returncode)}
        print(json.dumps(line))
        sys.exit(1)
    line[wl] = json.loads(got[0][len("RESULT "):])
print(json.dumps(line))
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "transform.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
