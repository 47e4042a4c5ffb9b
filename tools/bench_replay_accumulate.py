#!/usr/bin/env python3
"""The matches manager that accumulates over calls (eg3d_replay_accumulate, K8a) against the one-shot replay
(eg3d_replay_device, K8) on one GPU. One JSON line on stdout and profiles/replay_accumulate.json (EG3D_BENCH_OUT overrides
the path).

Per workload (C2 = Synth(2), C3' = Synth(3)) one child process under its own time limit (a fault or a hang of one workload
ends that child, and nothing is started after it). Inside it the seeds are matched device-only and the cloud is cut by seed
range into 1, 4 and 16 steps, each step's cloud kept in HBM as caller-built arrays; then, `reps` (>= 10) times after two
warm-up rounds:
  * eg3d_replay_device on the whole cloud, without the copy of the graph: the comparison the other numbers are read against;
  * per cut: every step's eg3d_replay_accumulate without materialisation (wall time at the C ABI, per step and summed), then
    one materialisation (an accumulate of an empty cloud that asks for the device graph), and the bytes of the state.
Also reported: whether the accumulated graph equals the one-shot graph bit for bit, and the node table's slots.

  python tools/bench_replay_accumulate.py [reps=10] [--workloads c2,c3] [--limit SECONDS]
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

ap = argparse.ArgumentParser(description="accumulating replay against the one-shot replay")
ap.add_argument("reps", nargs="?", type=int, default=10, help="repetitions (at least 10)")
ap.add_argument("--workloads", default="c2,c3", help="comma-separated: c2, c3")
ap.add_argument("--limit", type=int, default=400, help="time limit of one workload's child process, seconds")
ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
opt = ap.parse_args()
reps = max(10, opt.reps)
CONFIG = {"c2": 2, "c3": 3}
CUTS = (1, 4, 16)
ARRAYS = ("node_X", "node_point", "pl_start", "pl_end", "conn_off", "conn_pl", "iv_off", "iv_start_seg", "iv_start_xy",
          "iv_end_seg", "iv_end_xy")


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def worker(wl):
    from edgegraph3d_amd import _cdefs as D
    from edgegraph3d_amd import api, host
    L = api.lib()
    s = host.Synth(CONFIG[wl])
    ctx = api.Context(s.scene)
    ctx.upload_seeds(s.seeds)
    ns = s.n_seeds
    ctx.match_resident(0, ns, device_only=True)
    cloud = ctx.fetch_device_output()
    n = cloud["n_points"]
    seed_of = cloud["key"].reshape(-1, 4)[:, 0].astype(np.int64)

    def upload(a, b):
        """Points [a, b) of the cloud as caller-built device arrays."""
        off = cloud["obs_off"]
        o0, o1 = int(off[a]), int(off[b])
        arrays = {"X": cloud["X"][a:b], "obs_off": (off[a:b] - off[a]).astype(np.uint64), "obs_view": cloud["obs_view"][o0:o1],
                  "obs_pl": cloud["obs_pl"][o0:o1], "obs_seg": cloud["obs_seg"][o0:o1], "obs_xy": cloud["obs_xy"][o0:o1],
                  "key": cloud["key"][a:b]}
        held = {k: ctx.upload(v) for k, v in arrays.items()}
        d = D.DeviceEdgePoints()
        d.n_points, d.n_obs, d.complete = b - a, o1 - o0, 1
        for k, v in held.items():
            setattr(d, k, v.ptr)
        return d, held

    whole = upload(0, n)
    empty = D.DeviceEdgePoints()
    empty.complete = 1
    parts = {}
    for k in CUTS:
        edges = [int(np.searchsorted(seed_of, ns * i // k, side="left")) for i in range(k)] + [n]
        parts[k] = [upload(a, b) for a, b in zip(edges[:-1], edges[1:])]

    def one_shot(keep=False):
        st, dv = D.ReplayStats(), D.DeviceGraph3D()
        st.struct_size = C.sizeof(D.ReplayStats)
        t0 = time.perf_counter()
        assert L.eg3d_replay_device(ctx._h, C.byref(whole[0]), C.byref(dv), None, C.byref(st)) == 0
        ms = (time.perf_counter() - t0) * 1e3
        return {"ms": ms, "ms_graph": st.ms_graph, "ms_intervals": st.ms_intervals, "table_slots": int(st.table_slots),
                "pairs": int(st.n_pairs), "nodes": int(st.n_nodes), "polylines": int(st.n_polylines),
                "intervals": int(st.n_intervals), "result": ctx.fetch_device_graph(dv) if keep else None}

    def accumulated(k, keep=False):
        st, dv = D.ReplayStats(), D.DeviceGraph3D()
        st.struct_size = C.sizeof(D.ReplayStats)
        steps = []
        for i, (d, _) in enumerate(parts[k]):
            t0 = time.perf_counter()
            assert L.eg3d_replay_accumulate(ctx._h, C.byref(d), 1 if i == 0 else 0, None, None, C.byref(st)) == 0
            steps.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        assert L.eg3d_replay_accumulate(ctx._h, C.byref(empty), 0, C.byref(dv), None, C.byref(st)) == 0
        mat = (time.perf_counter() - t0) * 1e3
        return {"steps": steps, "sum": float(sum(steps)), "materialise": mat, "table_slots": int(st.table_slots),
                "state_bytes": ctx.replay_accumulated()["state_bytes"], "result": ctx.fetch_device_graph(dv) if keep else None}

    ref = one_shot(True)
    same = {}
    for k in CUTS:
        g = accumulated(k, True)["result"]
        same[k] = all(g[f] == ref["result"][f] for f in ("n_nodes", "n_real_nodes", "n_polylines")) and all(
            g[f].shape == ref["result"][f].shape and g[f].tobytes() == ref["result"][f].tobytes() for f in ARRAYS)
    one_shot()
    for k in CUTS:
        accumulated(k)
    a, b = [], {k: [] for k in CUTS}
    for _ in range(reps):
        a.append(one_shot())
        for k in CUTS:
            b[k].append(accumulated(k))
    sc = s.scene.contents
    r = {"workload": "%s (Synth(%d)): %d seeds, %d views, %d points, %d observations" % (wl, CONFIG[wl], ns, sc.n_views, n,
                                                                                           cloud["n_obs"]),
         "graph": {f: ref[f] for f in ("pairs", "nodes", "polylines", "intervals", "table_slots")},
         "one_shot_replay_device_ms": {f: stats([x[f] for x in a]) for f in ("ms", "ms_graph", "ms_intervals")},
         "accumulate": {}}
    for k in CUTS:
        r["accumulate"]["%d_steps" % k] = {
            "graph_bit_identical_to_one_shot": bool(same[k]),
            "sum_of_steps_ms": stats([x["sum"] for x in b[k]]),
            "per_step_ms": stats([t for x in b[k] for t in x["steps"]]),
            "materialise_ms": stats([x["materialise"] for x in b[k]]),
            "state_bytes": int(b[k][-1]["state_bytes"]), "table_slots": b[k][-1]["table_slots"],
            "sum_over_one_shot": float(np.median([x["sum"] for x in b[k]]) / np.median([x["ms"] for x in a]))}
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
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "replay_accumulate.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
