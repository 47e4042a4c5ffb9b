#!/usr/bin/env python3
"""K15, the colours of a resident cloud from the source images (include/eg3d_colour.h), against the two host routes a caller
has without it, on one GPU. One JSON line on stdout and profiles/colour.json (EG3D_BENCH_OUT overrides the path). No figure
here is a pass condition, and no speed-up is promised: the file is where the numbers go.

Per workload (c2 = Synth(2), c3 = Synth(3): C2, C3') one child process under its own time limit (a fault or a hang of one
workload ends that child, and nothing is started after it). The images are SEEDED RANDOM BYTES of the scene's size
(1600x1200), one per view, not photographs: the gather's locality, and with it the sampling time, may differ on real images.
After match_refpoints(device_only=True), for the resident cloud of that one step:
  upload_images_ms        the one-off eg3d_upload_images of all views (wall)
  colour_device           eg3d_colour_device(NULL) into preallocated arrays: wall time, ms_sample, ms_mix
  colours_d2h_ms          the copy of the colours alone, 3 bytes per point, to the host
  fetch_then_host_ms      route 1 of today: fetch_device_output() (the whole cloud to the host), then the host statement
                          on 16 threads; its two parts are reported as well
  host_statement_ms       route 2 of today: the host statement alone on a cloud that already is on the host
The comparison is against the host statement and against the copy the feature avoids, never against K15 itself. The GPU
result is compared with the host statement's, byte for byte, before its time is reported.

  python tools/bench_colour.py [reps=5] [--workloads c2,c3] [--limit SECONDS]
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

ap = argparse.ArgumentParser(description="K15 against the host routes")
ap.add_argument("reps", nargs="?", type=int, default=5)
ap.add_argument("--workloads", default="c2,c3")
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


def worker(wl):
    from edgegraph3d_amd import api, host
    s = host.Synth({"c2": 2, "c3": 3}[wl])
    sc = s.scene.contents
    V, W, H = int(sc.n_views), int(sc.width), int(sc.height)
    rng = np.random.default_rng(1500)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(V)]
    ctx = api.Context(s.scene)
    up_ms, _ = timed(lambda: ctx.upload_images(images))
    ctx.match_refpoints(s.seeds, device_only=True)
    n = int(ctx.last_device_output().n_points)
    rgb, flags = ctx.device_alloc(3 * n), ctx.device_alloc(n)
    st_all = []

    def call():
        st_all.append(ctx.colour_device(None, None, rgb, flags)[2])
    dev_ms, _ = timed(call)
    d2h_ms, got = timed(lambda: rgb.numpy(np.uint8, (n, 3)))
    fetch_ms, cloud = timed(ctx.fetch_device_output)
    args = (cloud["obs_off"].astype(np.uint32), cloud["obs_view"], cloud["obs_xy"])
    host_ms, want = timed(lambda: host.colour_points(images, *args, n_threads=HOST_THREADS))
    same = got.tobytes() == want[0].tobytes() and flags.numpy(np.uint8).tobytes() == want[1].tobytes()
    st = st_all[1:]
    g, h, f, c = stats(dev_ms), stats(host_ms), stats(fetch_ms), stats(d2h_ms)
    r = {"views": V, "image": [W, H], "images": "seeded random bytes, not photographs", "image_bytes": V * W * H * 3,
         "points": n, "observations": int(cloud["n_obs"]), "upload_images_ms": stats(up_ms),
         "colour_device": {"call_ms": g, "ms_sample": stats([x["ms_sample"] for x in st]), "ms_mix": stats([x["ms_mix"] for x in st])},
         "colours_d2h_ms": c, "fetch_device_output_ms": f, "host_statement_ms": h, "host_threads": HOST_THREADS,
         "fetch_then_host_ms": f["median"] + h["median"], "device_then_d2h_ms": g["median"] + c["median"],
         "host_statement_over_device_call": h["median"] / g["median"],
         "fetch_then_host_over_device_then_d2h": (f["median"] + h["median"]) / (g["median"] + c["median"]),
         "n_coloured": int(st[-1]["n_coloured"]), "n_empty": int(st[-1]["n_empty"]), "same_bytes_as_host_statement": bool(same)}
    ctx.close()
    s.close()
    print("RESULT " + json.dumps(r), flush=True)


if opt.worker:
    worker(opt.worker)
    sys.exit(0)

line = {"reps": reps, "host_threads": HOST_THREADS}
for wl in [w for w in opt.workloads.split(",") if w]:
    cmd = ["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), str(reps), "--worker", wl]
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
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "colour.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
