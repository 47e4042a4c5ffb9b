#!/usr/bin/env python3
"""The fundamental matrices from the tracks on the device (eg3d_estimate_fundamental, K12), on one GPU. One JSON line on
stdout and profiles/fundamental.json (EG3D_BENCH_OUT overrides the path).

Per workload (C2 = Synth(2), C3' = Synth(3), C4 = Synth(4)), one process: two warm-up calls, then `reps` (>= 10) device
calls. Reported: the stats struct of the first timed call, the medians of every stage time and of the wall time of the call
with their spread, the fit kernel's time per fit, and — the yardstick — ONE run each of the host statement
(eg3d_host_estimate_fundamental) and of eg3d_host_estimate_F on the cores this process is granted, in the same run.
The device result is compared with the host statement's bit for bit on the way (`equal_bits`).

  python tools/bench_fundamental.py [reps=10] [--workloads c2,c3,c4] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgegraph3d_amd import api, host  # noqa: E402

ap = argparse.ArgumentParser(description="fundamental matrices of all ordered view pairs on the device")
ap.add_argument("reps", nargs="?", type=int, default=10, help="timed device calls (at least 10)")
ap.add_argument("--workloads", default="c2,c3,c4", help="comma-separated: c2, c3, c4")
ap.add_argument("--no-host", action="store_true", help="skip the two host runs (no yardstick, no bit comparison)")
opt = ap.parse_args()
reps = max(10, opt.reps)
CONFIG = {"c2": 2, "c3": 3, "c4": 4}
SEED = 0xE63D2018
STAGES = ("ms_upload", "ms_lists", "ms_samples", "ms_fits", "ms_select", "ms_refit", "ms_copy")


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


line = {"reps": reps, "host_threads": int(os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0)))}
for wl in [w for w in opt.workloads.split(",") if w]:
    s = host.Synth(CONFIG[wl])
    V, ns = s.n_views, s.n_seeds
    for _ in range(2):
        F, valid, ncom, first = api.estimate_fundamental(V, s.seeds, rng_seed=SEED)
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        F, valid, ncom, st = api.estimate_fundamental(V, s.seeds, rng_seed=SEED)
        st["wall"] = (time.perf_counter() - t0) * 1e3
        runs.append(st)
    nc = ncom[valid != 0]
    rec = {"workload": "%s (Synth(%d)): %d seeds, %d views" % (wl, CONFIG[wl], ns, V),
           "stats": {k: int(v) for k, v in runs[0].items() if not k.startswith("ms_") and k not in ("wall", "struct_size")},
           "common_points": {"median": float(np.median(nc)) if len(nc) else 0.0, "max": int(nc.max()) if len(nc) else 0},
           "ms": {k: stats([r[k] for r in runs]) for k in STAGES + ("wall",)}}
    rec["ns_per_fit"] = 1e6 * rec["ms"]["ms_fits"]["median"] / max(1, rec["stats"]["n_fits"])
    if not opt.no_host:
        t0 = time.perf_counter()
        F0, valid0, ncom0, st0 = host.estimate_fundamental(V, s.seeds, rng_seed=SEED)
        rec["host_statement_ms"] = (time.perf_counter() - t0) * 1e3
        off, view, xy = s.seeds_np()
        t0 = time.perf_counter()
        host.estimate_F(V, off, view, xy, estimate=True, rng_seed=SEED)
        rec["host_estimate_F_ms"] = (time.perf_counter() - t0) * 1e3
        rec["equal_bits"] = bool(np.array_equal(F.view(np.uint64), F0.view(np.uint64)) and np.array_equal(valid, valid0)
                                 and np.array_equal(ncom, ncom0) and st0["n_fits_degenerate"] == runs[0]["n_fits_degenerate"]
                                 and st0["n_pairs_failed"] == runs[0]["n_pairs_failed"])
        rec["speedup_over_host_statement"] = rec["host_statement_ms"] / rec["ms"]["wall"]["median"]
    line[wl] = rec
    s.close()
print(json.dumps(line))
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "fundamental.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
