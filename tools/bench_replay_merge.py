#!/usr/bin/env python3
"""The matches manager merging the graphs of later shards (eg3d_replay_merge_graph, K8m) on one GPU, against the two ways the
same graph is had without it: eg3d_replay_accumulate over the shards' clouds in order, and eg3d_replay_device on the one-call
cloud. One JSON line on stdout and profiles/replay_merge.json (EG3D_BENCH_OUT overrides the path).

Per workload (C2 = Synth(2), C3' = Synth(3)) one child process under its own time limit (a fault or a hang of one workload
ends that child, and nothing is started after it). Inside it the seeds are matched device-only and the cloud is cut by seed
range into 2, 4 and 8 shards, each kept in HBM as caller-built arrays and replayed once on a clone of its own
(eg3d_replay_device: the graph stays in that clone's buffers). Then, `reps` (>= 10) times after two warm-up rounds, wall time
at the C ABI:
  * the fold: eg3d_replay_merge_graph of the shards' graphs in order into the first context's accumulator, the last call
    materialising the device graph;
  * eg3d_replay_accumulate over the same clouds in order, the last call materialising;
  * eg3d_replay_device on the one-call cloud, without the copy of the graph;
  * once per shard, its eg3d_replay_device on the clone (what a rank or lane pays before it has a graph to contribute).
Also reported: the bytes of the shards' graphs as the merge reads them next to the bytes of the clouds they stand for, and
whether the folded graph equals the one-shot graph bit for bit. One GPU: the exchange between ranks is not measured here.

  python tools/bench_replay_merge.py [reps=10] [--workloads c2,c3] [--limit SECONDS]
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

ap = argparse.ArgumentParser(description="merging the graphs of shards against accumulating their clouds")
ap.add_argument("reps", nargs="?", type=int, default=10, help="repetitions (at least 10)")
ap.add_argument("--workloads", default="c2,c3", help="comma-separated: c2, c3")
ap.add_argument("--limit", type=int, default=400, help="time limit of one workload's child process, seconds")
ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
opt = ap.parse_args()
reps = max(10, opt.reps)
CONFIG = {"c2": 2, "c3": 3}
CUTS = (2, 4, 8)
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
    n_scene_pl = int(s.scene_np()["view_pl_off"][-1])

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

    def new_stats():
        st = D.ReplayStats()
        st.struct_size = C.sizeof(D.ReplayStats)
        return st

    whole = upload(0, n)
    clones = [ctx.clone() for _ in range(max(CUTS))]
    parts, graphs, sizes = {}, {}, {}
    for k in CUTS:
        edges = [int(np.searchsorted(seed_of, ns * i // k, side="left")) for i in range(k)] + [n]
        parts[k] = [upload(a, b) for a, b in zip(edges[:-1], edges[1:])]

    def replay_shards(k):
        """Every shard of the cut on its own clone: [(DeviceGraph3D, points, pairs)], the wall time of each."""
        out, ms = [], []
        for i, (d, _) in enumerate(parts[k]):
            st, dv = new_stats(), D.DeviceGraph3D()
            t0 = time.perf_counter()
            assert L.eg3d_replay_device(clones[i]._h, C.byref(d), C.byref(dv), None, C.byref(st)) == 0
            ms.append((time.perf_counter() - t0) * 1e3)
            out.append((dv, int(d.n_points), int(st.n_pairs), int(st.n_intervals)))
        return out, ms

    def one_shot(keep=False):
        st, dv = new_stats(), D.DeviceGraph3D()
        t0 = time.perf_counter()
        assert L.eg3d_replay_device(ctx._h, C.byref(whole[0]), C.byref(dv), None, C.byref(st)) == 0
        ms = (time.perf_counter() - t0) * 1e3
        return {"ms": ms, "pairs": int(st.n_pairs), "nodes": int(st.n_nodes), "polylines": int(st.n_polylines),
                "intervals": int(st.n_intervals), "result": ctx.fetch_device_graph(dv) if keep else None}

    def folded(k, keep=False):
        st, dv = new_stats(), D.DeviceGraph3D()
        steps = []
        for i, (g, pts, pairs, _) in enumerate(graphs[k]):
            last = i == k - 1
            t0 = time.perf_counter()
            assert L.eg3d_replay_merge_graph(ctx._h, C.byref(g), pts, pairs, 1 if i == 0 else 0, C.byref(dv) if last else None, None,
                                             C.byref(st)) == 0
            steps.append((time.perf_counter() - t0) * 1e3)
        return {"steps": steps, "sum": float(sum(steps)), "table_slots": int(st.table_slots),
                "result": ctx.fetch_device_graph(dv) if keep else None}

    def accumulated(k):
        st, dv = new_stats(), D.DeviceGraph3D()
        steps = []
        for i, (d, _) in enumerate(parts[k]):
            last = i == k - 1
            t0 = time.perf_counter()
            assert L.eg3d_replay_accumulate(ctx._h, C.byref(d), 1 if i == 0 else 0, C.byref(dv) if last else None, None, C.byref(st)) == 0
            steps.append((time.perf_counter() - t0) * 1e3)
        return {"steps": steps, "sum": float(sum(steps))}

    ref = one_shot(True)
    same, shard_ms = {}, {}
    for k in CUTS:
        graphs[k], _ = replay_shards(k)
        g = folded(k, True)["result"]
        same[k] = all(g[f] == ref["result"][f] for f in ("n_nodes", "n_real_nodes", "n_polylines")) and all(
            g[f].shape == ref["result"][f].shape and g[f].tobytes() == ref["result"][f].tobytes() for f in ARRAYS)
        # what the merge reads of a graph: nodes (X, point), polylines (two ends), the interval table
        sizes[k] = {
            "graph_bytes": int(sum(20 * int(g.n_nodes) + 8 * int(g.n_polylines) + 8 * (n_scene_pl + 1) + 24 * iv for g, _, _, iv in graphs[k])),
            "cloud_bytes": int(sum(36 * int(d.n_points) + 20 * int(d.n_obs) for d, _ in parts[k])),
            "sum_of_shard_nodes": int(sum(int(g.n_nodes) for g, *_ in graphs[k])),
            "sum_of_shard_polylines": int(sum(int(g.n_polylines) for g, *_ in graphs[k])),
            "sum_of_shard_intervals": int(sum(iv for *_, iv in graphs[k]))}
        accumulated(k)
        folded(k)
    one_shot()
    a, f, b = [], {k: [] for k in CUTS}, {k: [] for k in CUTS}
    for k in CUTS:
        shard_ms[k] = []
    for _ in range(reps):
        a.append(one_shot())
        for k in CUTS:
            graphs[k], ms = replay_shards(k)
            shard_ms[k].extend(ms)
            f[k].append(folded(k))
            b[k].append(accumulated(k))
    sc = s.scene.contents
    r = {"workload": "%s (Synth(%d)): %d seeds, %d views, %d points, %d observations" % (wl, CONFIG[wl], ns, sc.n_views, n,
                                                                                           cloud["n_obs"]),
         "graph": {k: ref[k] for k in ("pairs", "nodes", "polylines", "intervals")},
         "one_shot_replay_device_ms": stats([x["ms"] for x in a]), "shards": {}}
    for k in CUTS:
        r["shards"]["%d" % k] = dict(sizes[k], **{
            "graph_bit_identical_to_one_shot": bool(same[k]),
            "fold_ms": stats([x["sum"] for x in f[k]]),
            "fold_per_merge_ms": stats([t for x in f[k] for t in x["steps"]]),
            "accumulate_same_clouds_ms": stats([x["sum"] for x in b[k]]),
            "shard_replay_on_clone_ms": stats(shard_ms[k]),
            "table_slots": f[k][-1]["table_slots"],
            "fold_over_accumulate": float(np.median([x["sum"] for x in f[k]]) / np.median([x["sum"] for x in b[k]])),
            "graph_bytes_over_cloud_bytes": sizes[k]["graph_bytes"] / max(1, sizes[k]["cloud_bytes"])})
    for c in clones:
        c.close()
    ctx.close()
    s.close()
    print("RESULT " + json.dumps(r), flush=True)


if opt.worker:
    worker(opt.worker)
    sys.exit(0)

line = {"reps": reps, "note": "one GPU; the exchange of the graphs between ranks is not measured"}
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
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "replay_merge.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
