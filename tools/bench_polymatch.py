#!/usr/bin/env python3
"""Pipeline 2's polyline matcher on the device (eg3d_match_polylines_closeness), on one GPU. One JSON line on stdout and
profiles/polymatch.json (EG3D_BENCH_OUT overrides the path).

Per workload (C2 = Synth(2), C3' = Synth(3)), one process: the first call builds the 10 px map (ms_grid is reported from that
call only), a second call is the other warm-up, then `reps` (>= 10) calls on the uploaded seeds. Reported: the medians of
ms_search (the search kernel), ms_components (rule, union-find, the two sorts, CSR, compaction), ms_copy and the wall time of
the call, each with its spread, and the entry, accepted, node and set counts.

  python tools/bench_polymatch.py [reps=10] [--workloads c2,c3]
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

ap = argparse.ArgumentParser(description="polyline matching by closeness to the reference points on the device")
ap.add_argument("reps", nargs="?", type=int, default=10, help="timed calls (at least 10)")
ap.add_argument("--workloads", default="c2,c3", help="comma-separated: c2, c3")
opt = ap.parse_args()
reps = max(10, opt.reps)
CONFIG = {"c2": 2, "c3": 3}


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


line = {"reps": reps}
for wl in [w for w in opt.workloads.split(",") if w]:
    s = host.Synth(CONFIG[wl])
    ctx = api.Context(s.scene)
    ctx.upload_seeds(s.seeds)
    ns = s.n_seeds
    first = ctx.match_polylines_closeness(None, 0, ns)["stats"]   # builds the 10 px map
    ctx.match_polylines_closeness(None, 0, ns)
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        st = ctx.match_polylines_closeness(None, 0, ns)["stats"]
        st["wall"] = (time.perf_counter() - t0) * 1e3
        runs.append(st)
    line[wl] = {"workload": "%s (Synth(%d)): %d seeds, %d views" % (wl, CONFIG[wl], ns, s.n_views),
                "n_entries": int(first["n_entries"]), "n_accepted": int(first["n_accepted"]),
                "n_nodes": int(first["n_nodes"]), "n_sets": int(first["n_sets"]), "ms_grid_first_call": first["ms_grid"],
                "ms": {k: stats([r[k] for r in runs]) for k in ("ms_search", "ms_components", "ms_copy", "wall")}}
    ctx.close()
    s.close()
print(json.dumps(line))
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "polymatch.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
