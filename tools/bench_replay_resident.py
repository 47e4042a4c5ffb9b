#!/usr/bin/env python3
"""The PLGMatchesManager replay (row a17) on the device against the replay on the host, on one GPU. One JSON line on stdout
and profiles/replay_resident.json (EG3D_BENCH_OUT overrides the path).

Per workload (C2 = Synth(2), C3' = Synth(3)) one child process under its own time limit (a fault or a hang of one workload
ends that child, and nothing is started after it); inside it, on one context and one cloud, two warm-up rounds, then `reps`
(>= 10) repetitions of each path, alternating:
  (a) parent: eg3d_match_resident with the copy of the whole cloud -> eg3d_host_replay_matches (host/replay.cpp);
  (b) new:    device-only match -> eg3d_replay_device with the copy of the graph.
Both are timed at the C ABI. Reported: both medians with their spread, the HIP-event times of the graph and interval stages,
the size of the graph, and whether the two graphs are identical bit for bit.

  python tools/bench_replay_resident.py [reps=10] [--workloads c2,c3] [--limit SECONDS]
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

ap = argparse.ArgumentParser(description="replay on the device against the replay on the host")
ap.add_argument("reps", nargs="?", type=int, default=10, help="repetitions of each path (at least 10)")
ap.add_argument("--workloads", default="c2,c3", help="comma-separated: c2, c3")
ap.add_argument("--limit", type=int, default=400, help="time limit of one workload's child process, seconds")
ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
opt = ap.parse_args()
reps = max(10, opt.reps)
CONFIG = {"c2": 2, "c3": 3}
ARRAYS = ("node_X", "node_point", "pl_start", "pl_end", "conn_off", "conn_pl", "iv_off", "iv_start_seg", "iv_start_xy",
          "iv_end_seg", "iv_end_xy")


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def worker(wl):
    from edgegraph3d_amd import _cdefs as D
    from edgegraph3d_amd import api, host
    L, H = api.lib(), host.lib()
    s = host.Synth(CONFIG[wl])
    sc = s.scene.contents
    ctx = api.Context(s.scene)
    ctx.upload_seeds(s.seeds)
    ns = s.n_seeds

    def host_path(keep_result=False):
        t0 = time.perf_counter()
        e, tm = D.EdgePoints(), D.StageTimes()
        assert L.eg3d_match_resident(ctx._h, 0, ns, 0, C.byref(e), C.byref(tm)) == 0
        t1 = time.perf_counter()
        g = D.Graph3D()
        assert H.eg3d_host_replay_matches(s.scene, C.byref(e), C.byref(g)) == 0
        t2 = time.perf_counter()
        res = D.graph3d_to_dict(g) if keep_result else None
        n, m = int(e.n_points), int(e.n_obs)
        H.eg3d_host_free_graph3d(C.byref(g))
        L.eg3d_free_edgepoints(C.byref(e))
        return {"total": (t2 - t0) * 1e3, "match_to_host": (t1 - t0) * 1e3, "host_replay": (t2 - t1) * 1e3, "n": n, "m": m,
                "result": res}

    def resident_path(keep_result=False):
        t0 = time.perf_counter()
        e, tm = D.EdgePoints(), D.StageTimes()
        assert L.eg3d_match_resident(ctx._h, 0, ns, 1, C.byref(e), C.byref(tm)) == 0
        t1 = time.perf_counter()
        g, st = D.Graph3D(), D.ReplayStats()
        st.struct_size = C.sizeof(D.ReplayStats)
        assert L.eg3d_replay_device(ctx._h, None, None, C.byref(g), C.byref(st)) == 0
        t2 = time.perf_counter()
        res = D.graph3d_to_dict(g) if keep_result else None
        nc = int(g.conn_off[int(g.n_nodes)])
        L.eg3d_free_graph3d(C.byref(g))
        return {"total": (t2 - t0) * 1e3, "match_device_only": (t1 - t0) * 1e3, "replay_device": (t2 - t1) * 1e3,
                "ms_graph": st.ms_graph, "ms_intervals": st.ms_intervals, "ms_copy": st.ms_copy, "pairs": int(st.n_pairs),
                "nodes": int(st.n_nodes), "polylines": int(st.n_polylines), "intervals": int(st.n_intervals),
                "connections": nc, "table_slots": int(st.table_slots), "result": res}

    a0, b0 = host_path(True), resident_path(True)   # warm-up, and the comparison
    ga, gb = a0["result"], b0["result"]
    same = all(ga[f] == gb[f] for f in ("n_nodes", "n_real_nodes", "n_polylines")) and all(
        ga[f].shape == gb[f].shape and ga[f].tobytes() == gb[f].tobytes() for f in ARRAYS)
    host_path(), resident_path()                    # the host call's pipelining lanes exist now
    ha, rb = [], []
    for _ in range(reps):
        ha.append(host_path())
        rb.append(resident_path())
    n, m, NP = a0["n"], a0["m"], int(sc.view_pl_off[sc.n_views])
    graph_bytes = (20 * b0["nodes"] + 8 * (b0["nodes"] + 1) + 8 * b0["polylines"] + 4 * b0["connections"] + 8 * (NP + 1)
                   + 24 * b0["intervals"])
    r = {"workload": "%s (Synth(%d)): %d seeds, %d views, %d points, %d observations" % (wl, CONFIG[wl], ns, sc.n_views, n, m),
         "graph": {k: b0[k] for k in ("pairs", "nodes", "polylines", "connections", "intervals", "table_slots")},
         "graphs_bit_identical": bool(same),
         "a_parent_path_ms": {k: stats([x[k] for x in ha]) for k in ("total", "match_to_host", "host_replay")},
         "b_new_path_ms": {k: stats([x[k] for x in rb]) for k in ("total", "match_device_only", "replay_device", "ms_graph",
                                                                  "ms_intervals", "ms_copy")},
         "a_d2h_bytes": 36 * n + 8 + 20 * m, "b_d2h_bytes": graph_bytes}
    r["speedup_total"] = r["a_parent_path_ms"]["total"]["median"] / r["b_new_path_ms"]["total"]["median"]
    ctx.close()
    s.close()
    print("RESULT " + json.dumps(r), flush=True)


if opt.worker:
    worker(opt.worker)
    sys.exit(0)

line = {"reps": reps}
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
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "replay_resident.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
