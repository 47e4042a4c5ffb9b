#!/usr/bin/env python3
"""K17, the 3-D edge model of a resident graph (include/eg3d/edges.h), against the route a caller has without it: copy the
graph to the host and run eg3d_host_edge_chains there. One GPU. One JSON line on stdout and profiles/edges.json
(EG3D_BENCH_OUT overrides the path). No figure here is a pass condition, and no ratio is promised: the file is where the
numbers go.

Per workload one child process under its own time limit (a fault or a hang of one workload ends that child, and nothing is
started after it):
  c2, c3    the graph eg3d_replay_device leaves resident for host.Synth(2) / Synth(3) (C2, C3') after
            match_refpoints(device_only=True)
For each, medians of `reps` (10) repetitions after 2 warm-ups:
  device        eg3d_edge_chains_device with the copy of the model to the host: wall time of the call, and the call's own
                ms_trace, ms_simplify, ms_copy
  host_route    the geometric half of the graph device -> host (node_X, pl_start, pl_end, conn_off, conn_pl), then
                eg3d_host_edge_chains: the two parts and their sum
The device result is compared with the host statement's, byte for byte, before its time is reported. Printed as well:
chains, rings, the longest chain, vertices in and kept.

  python tools/bench_edges.py [reps=10] [--workloads c2,c3] [--max-dist 0.01] [--limit SECONDS]
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

ap = argparse.ArgumentParser(description="K17 against copy-the-graph + the host statement")
ap.add_argument("reps", nargs="?", type=int, default=10)
ap.add_argument("--workloads", default="c2,c3")
ap.add_argument("--max-dist", type=float, default=0.01)
ap.add_argument("--limit", type=int, default=300, help="time limit of one workload's child process, seconds")
ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
opt = ap.parse_args()
reps = max(3, opt.reps)
WARMUPS = 2
ARRAYS = ("chain_off", "chain_node", "flags", "s_off", "s_node", "length")
COUNTS = ("n_chains", "n_rings", "n_loops_dropped", "n_vertices_in", "n_vertices_kept", "longest_chain")


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


def worker(wl):
    from edgegraph3d_amd import api, host
    s = host.Synth({"c2": 2, "c3": 3}[wl])
    ctx = api.Context(s.scene)
    r = ctx.match_refpoints(s.seeds, device_only=True)
    _, dv, rst = ctx.replay_device(to_host=False)
    runs = []
    dev_ms, got = timed(lambda: runs.append(ctx.edge_chains_device(dv, max_dist=opt.max_dist)) or runs[-1])
    copy_ms, graph = timed(lambda: ctx.fetch_device_graph(dv))   # (all of the graph: the interval half is a small part of it)
    host_ms, want = timed(lambda: host.edge_chains(graph, opt.max_dist))
    same = all(got[k].tobytes() == want[k].tobytes() for k in ARRAYS) and all(got["stats"][k] == want["stats"][k] for k in COUNTS)
    d, a, b = stats(dev_ms), stats(copy_ms), stats(host_ms)
    out = {"points": int(r["n_points"]), "nodes": int(rst["n_nodes"]), "polylines": int(rst["n_polylines"]), "max_dist": opt.max_dist}
    out.update({k: int(got["stats"][k]) for k in COUNTS})
    out.update({"device": {"call_ms": d, **{k: stats([x["stats"][k] for x in runs[WARMUPS:]]) for k in ("ms_trace", "ms_simplify", "ms_copy")}},
                "host_route": {"graph_to_host_ms": a, "host_statement_ms": b, "sum_of_medians_ms": a["median"] + b["median"]},
                "host_route_over_device_call": (a["median"] + b["median"]) / d["median"], "same_bytes_as_host_statement": bool(same)})
    ctx.close()
    s.close()
    print("RESULT " + json.dumps(out), flush=True)


if opt.worker:
    worker(opt.worker)
    sys.exit(0)

line = {"reps": reps, "warmups": WARMUPS}
for wl in [w for w in opt.workloads.split(",") if w]:
    cmd = ["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), str(reps), "--worker", wl, "--max-dist",
           str(opt.max_dist)]
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
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "edges.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
