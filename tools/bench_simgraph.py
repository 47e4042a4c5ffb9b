#!/usr/bin/env python3
"""Pipeline 1's polyline compatibility graph on the device (eg3d_similarity_graph), on one GPU. One JSON line on stdout and
profiles/simgraph.json (EG3D_BENCH_OUT overrides the path).

Per workload (C2 = Synth(2), C3' = Synth(3)), one process: the first call builds the 10 px map (ms_grid is reported from that
call only), a second call is the other warm-up, then `reps` (>= 10) calls on the uploaded seeds. Reported: the medians of
ms_search (count, scan, fill), ms_graph (the lists, the nodes, the distinct edges), ms_weights (edge weights and the
adjacency), ms_copy and the wall time of the call, each with its spread, and the entry, node, edge, pair-instance and chunk
counts. No host form of this stage exists in the project: no ratio is reported.

  python tools/bench_simgraph.py [reps=10] [--workloads c2,c3]
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

ap = argparse.ArgumentParser(description="the polyline compatibility graph of pipeline 1 on the device")
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
    first = ctx.similarity_graph(None, 0, ns)   # builds the 10 px map
    ctx.similarity_graph(None, 0, ns)
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        st = ctx.similarity_graph(None, 0, ns)["stats"]
        st["wall"] = (time.perf_counter() - t0) * 1e3
        runs.append(st)
    f = first["stats"]
    line[wl] = {"workload": "%s (Synth(%d)): %d seeds, %d views" % (wl, CONFIG[wl], ns, s.n_views),
                "n_entries": int(f["n_entries"]), "n_nodes": int(f["n_nodes"]), "n_edges": int(f["n_edges"]),
                "n_pair_instances": int(f["n_pair_instances"]), "n_chunks": int(f["n_chunks"]),
                "n_close_pairs": int(first["cp_off"][-1]), "max_close_refpoints_row": int(np.diff(first["cr_off"]).max()),
                "ms_grid_first_call": f["ms_grid"],
                "ms": {k: stats([r[k] for r in runs]) for k in ("ms_search", "ms_graph", "ms_weights", "ms_copy", "wall")}}
    ctx.close()
    s.close()
print(json.dumps(line))
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "simgraph.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as fo:
    json.dump(line, fo, indent=1)
    fo.write("\n")
