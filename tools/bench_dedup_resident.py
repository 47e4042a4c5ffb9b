#!/usr/bin/env python3
"""The 3 px dedup on the device against the dedup on the host, on one GPU. One JSON line on stdout and
profiles/dedup_resident.json (EG3D_BENCH_OUT overrides the path).

Per workload (C2 = Synth(2), C3' = Synth(3)), one process, two warm-up rounds, then `reps` (>= 10) repetitions of each
path, alternating:
  (a) the path through the host: eg3d_match_resident with the copy of the whole cloud -> eg3d_host_filter_close_2d;
  (b) the resident path: device-only match -> eg3d_dedup_resident (dedup, compaction, copy of the survivors).
Both are timed at the C ABI. Reported: both medians with their spread, the HIP-event time of the two dedup kernels, the
kept share, and whether the clouds of the two paths (the numpy compaction of (a)'s cloud by its mask against (b)'s
survivors) are identical bit for bit.

  python tools/bench_dedup_resident.py [reps=10] [--workloads c2,c3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgegraph3d_amd import _cdefs as D  # noqa: E402
from edgegraph3d_amd import api, host  # noqa: E402
from edgegraph3d_amd.cloudnp import np_compact, same_cloud  # noqa: E402

ap = argparse.ArgumentParser(description="3 px dedup on the device against the dedup on the host")
ap.add_argument("reps", nargs="?", type=int, default=10, help="repetitions of each path (at least 10)")
ap.add_argument("--workloads", default="c2,c3", help="comma-separated: c2, c3")
opt = ap.parse_args()
reps, workloads = max(10, opt.reps), opt.workloads
L, H = api.lib(), host.lib()
CONFIG = {"c2": 2, "c3": 3}


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def host_path(ctx, sc, n_seeds, keep_result=False):
    t0 = time.perf_counter()
    e, tm = D.EdgePoints(), D.StageTimes()
    assert L.eg3d_match_resident(ctx._h, 0, n_seeds, 0, C.byref(e), C.byref(tm)) == 0
    t1 = time.perf_counter()
    n, m = int(e.n_points), int(e.n_obs)
    keep = np.empty(max(n, 1), np.uint8)
    assert H.eg3d_host_filter_close_2d(sc.n_views, sc.width, sc.height, C.byref(e), D.np_ptr(keep, C.c_uint8)) == 0
    t2 = time.perf_counter()
    res = None
    if keep_result:
        res = np_compact(D.edgepoints_to_dict(e), keep[:n])
    L.eg3d_free_edgepoints(C.byref(e))
    return {"total": (t2 - t0) * 1e3, "match_to_host": (t1 - t0) * 1e3, "host_dedup": (t2 - t1) * 1e3, "n": n, "m": m,
            "kept": int(keep[:n].sum()), "result": res}


def resident_path(ctx, n_seeds, keep_result=False):
    t0 = time.perf_counter()
    e, tm = D.EdgePoints(), D.StageTimes()
    assert L.eg3d_match_resident(ctx._h, 0, n_seeds, 1, C.byref(e), C.byref(tm)) == 0
    t1 = time.perf_counter()
    o, st = D.EdgePoints(), D.DedupStats()
    st.struct_size = C.sizeof(D.DedupStats)
    assert L.eg3d_dedup_resident(ctx._h, 0, 1, 0, 0.0, 0, -1, None, 1, C.byref(o), None, C.byref(st)) == 0
    t2 = time.perf_counter()
    res = D.edgepoints_to_dict(o) if keep_result else None
    L.eg3d_free_edgepoints(C.byref(o))
    return {"total": (t2 - t0) * 1e3, "match_device_only": (t1 - t0) * 1e3, "dedup_resident": (t2 - t1) * 1e3,
            "ms_dedup": st.ms_dedup, "ms_compact": st.ms_compact, "ms_copy": st.ms_copy, "kept": int(st.n_kept),
            "obs_kept": int(st.n_obs_kept), "result": res}


line = {"reps": reps}
for wl in [w for w in workloads.split(",") if w]:
    s = host.Synth(CONFIG[wl])
    sc = s.scene.contents
    ctx = api.Context(s.scene)
    ctx.upload_seeds(s.seeds)
    ns = s.n_seeds
    a0, b0 = host_path(ctx, sc, ns, True), resident_path(ctx, ns, True)   # warm-up, and the comparison
    same = same_cloud(a0["result"], b0["result"]) is None and a0["kept"] == b0["kept"]
    host_path(ctx, sc, ns), resident_path(ctx, ns)                         # the host call's pipelining lanes exist now
    ha, rb = [], []
    for _ in range(reps):
        ha.append(host_path(ctx, sc, ns))
        rb.append(resident_path(ctx, ns))
    n, m = a0["n"], a0["m"]
    w, h = int(np.ceil(np.float32(sc.width) / np.float32(3))), int(np.ceil(np.float32(sc.height) / np.float32(3)))
    r = {"workload": "%s (Synth(%d)): %d seeds, %d views, %d points, %d observations" % (wl, CONFIG[wl], ns, sc.n_views, n, m),
         "kept_points": a0["kept"], "kept_share": a0["kept"] / max(n, 1), "kept_observations": b0["obs_kept"],
         "clouds_bit_identical": bool(same), "claim_map_bytes": 4 * sc.n_views * w * h,
         "a_host_path_ms": {k: stats([x[k] for x in ha]) for k in ("total", "match_to_host", "host_dedup")},
         "b_resident_path_ms": {k: stats([x[k] for x in rb]) for k in ("total", "match_device_only", "dedup_resident",
                                                                      "ms_dedup", "ms_compact", "ms_copy")},
         "a_d2h_bytes": 36 * n + 8 + 20 * m, "b_d2h_bytes": 36 * a0["kept"] + 20 * b0["obs_kept"] + 40}
    r["speedup_total"] = r["a_host_path_ms"]["total"]["median"] / r["b_resident_path_ms"]["total"]["median"]
    line[wl] = r
    ctx.close()
    s.close()
print(json.dumps(line))
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "dedup_resident.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
