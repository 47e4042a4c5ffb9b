#!/usr/bin/env python3
"""Pipeline 1's community detection on the device (eg3d_detect_communities, K11), on one GPU. One JSON line on stdout and
profiles/louvain.json (EG3D_BENCH_OUT overrides the path).

Per workload (C2 = Synth(2), C3' = Synth(3)), one process: the compatibility graph is built once (eg3d_similarity_graph), two
warm-up calls, then `reps` (>= 10) calls on the same graph. Reported: the medians of ms_upload (the copy of the graph and its
checks), ms_sweeps, ms_coarsen (renumbering and the coarse graphs), ms_copy and the wall time of the call, each with its
spread, and the sweeps, phases, communities, modularity and overflow rows. Every stage of K11 ends in a read-back that
synchronises the stream, so the stage times are the library's host clock between those points, not HIP events. No host form
of this stage exists in the project: no ratio is reported.

  python tools/bench_louvain.py [reps=10] [--workloads c2,c3]
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

ap = argparse.ArgumentParser(description="the community detection of pipeline 1 on the device")
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
    g = ctx.similarity_graph(None, 0, s.n_seeds)
    first = ctx.communities(g)
    ctx.communities(g)
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = ctx.communities(g)
        st = r["stats"]
        st["wall"] = (time.perf_counter() - t0) * 1e3
        assert r["ids"].tobytes() == first["ids"].tobytes()
        runs.append(st)
    f = first["stats"]
    line[wl] = {"workload": "%s (Synth(%d)): %d seeds, %d views" % (wl, CONFIG[wl], s.n_seeds, s.n_views),
                "n_nodes": int(g["n_nodes"]), "n_entries": int(g["adj_off"][-1]), "max_row": int(np.diff(g["adj_off"]).max()),
                "n_phases": int(f["n_phases"]), "n_sweeps": int(f["n_sweeps"]), "n_communities": int(f["n_communities"]),
                "n_isolated": int(f["n_isolated"]), "n_overflow_rows": int(f["n_overflow_rows"]), "modularity": f["modularity"],
                "ms": {k: stats([r[k] for r in runs]) for k in ("ms_upload", "ms_sweeps", "ms_coarsen", "ms_copy", "wall")}}
    ctx.close()
    s.close()
print(json.dumps(line))
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "louvain.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as fo:
    json.dump(line, fo, indent=1)
    fo.write("\n")
