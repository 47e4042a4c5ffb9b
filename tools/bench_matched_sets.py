#!/usr/bin/env python3
"""The pipelines 1-2 extractor without and with a filled PLGMatchesManager, on one GPU. One JSON line on stdout and
profiles/matched_sets.json (EG3D_BENCH_OUT overrides the path).

Per workload (C2 = Synth(2), C3' = Synth(3); the sets are the workload's curve sets, as bench.py --path sets) one child
process under its own time limit (a fault or a hang of one workload ends that child, and nothing is started after it).
Inside it, on one context:
  1. pipeline 3, device only, and eg3d_replay_device: the matched intervals stay in HBM (their cost is reported: it precedes
     the extractor in a run that wants them);
  2. stage A alone, without and with the intervals (eg3d_polyline_set_candidates): samples, tasks, skipped, hits filtered;
  3. two warm-up rounds, then `reps` (>= 10) repetitions, alternating, of
       (a) eg3d_match_polyline_sets                       — the unchanged path: compare with bench.py --path sets of the parent
       (b) eg3d_match_polyline_sets_matched, m = NULL     — must be (a)
       (c) eg3d_match_polyline_sets_matched, device intervals
     each with the copy of its cloud, timed at the C ABI; medians with their spread, the HIP-event stage times of (a) and (c).

  python tools/bench_matched_sets.py [reps=10] [--workloads c2,c3] [--limit SECONDS]
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

ap = argparse.ArgumentParser(description="the extractor without and with the matches manager")
ap.add_argument("reps", nargs="?", type=int, default=10, help="repetitions of each path (at least 10)")
ap.add_argument("--workloads", default="c2,c3", help="comma-separated: c2, c3")
ap.add_argument("--limit", type=int, default=400, help="time limit of one workload's child process, seconds")
ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
opt = ap.parse_args()
reps = max(10, opt.reps)
CONFIG = {"c2": 2, "c3": 3}
STAGES = ("ms_total", "ms_candidates", "ms_epipolar", "ms_hypotheses", "ms_select", "ms_expand", "ms_emit")


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def worker(wl):
    from edgegraph3d_amd import _cdefs as D
    from edgegraph3d_amd import api, host
    L = api.lib()
    s = host.Synth(CONFIG[wl])
    ctx = api.Context(s.scene)
    n, row_off, ids = s.polyline_sets()
    row_off = np.ascontiguousarray(row_off, np.uint32)
    ids = np.ascontiguousarray(ids if len(ids) else [0], np.uint32)
    ps = D.PolylineSets(n, D.np_ptr(row_off, C.c_uint32), D.np_ptr(ids, C.c_uint32))

    # 1. what precedes the extractor: pipeline 3 and the replay, both on the device
    ctx.upload_seeds(s.seeds)
    prior = []
    for _ in range(3):
        t0 = time.perf_counter()
        cloud = ctx.match_resident(0, s.n_seeds, device_only=True)
        t1 = time.perf_counter()
        _, dv, rst = ctx.replay_device(to_host=False)
        t2 = time.perf_counter()
        prior.append({"match_device_only": (t1 - t0) * 1e3, "replay_device": (t2 - t1) * 1e3})
    held = D.MatchedIntervalsArrays(dv)

    # 2. the counts
    try:
        c0 = ctx.polyline_set_candidates(n, row_off, ids)
        c1 = ctx.polyline_set_candidates(n, row_off, ids, matched=held)
        counts = {"samples": c0["n_tasks"], "hits": int(c0["list_off"][-1]) - c0["n_tasks"], "tasks_with_manager": c1["n_tasks"],
                  "samples_skipped": c1["n_samples_skipped"], "hits_filtered": c1["n_hits_filtered"],
                  "hits_with_manager": int(c1["list_off"][-1]) - c1["n_tasks"]}
    except api.Eg3dError as ex:  # (stage A alone runs the whole range as one batch: too many samples for that)
        counts = {"error": str(ex)}

    # 3. the calls
    def call(which):
        e, tm = D.EdgePoints(), D.StageTimes()
        t0 = time.perf_counter()
        if which == "a":
            rc = L.eg3d_match_polyline_sets(ctx._h, C.byref(ps), 0, n, 0, C.byref(e), C.byref(tm))
        else:
            rc = L.eg3d_match_polyline_sets_matched(ctx._h, C.byref(ps), 0, n, C.byref(held.c) if which == "c" else None, 0,
                                                    C.byref(e), C.byref(tm))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, L.eg3d_last_error()
        r = {"end_to_end": dt, "points": int(e.n_points), "obs": int(e.n_obs), "tasks": int(e.n_tasks), "chains": int(e.n_chains)}
        r.update({k: float(getattr(tm, k)) for k in STAGES})
        L.eg3d_free_edgepoints(C.byref(e))
        return r

    for _ in range(2):
        for w in "abc":
            call(w)
    runs = {w: [] for w in "abc"}
    for _ in range(reps):
        for w in "abc":
            runs[w].append(call(w))
    sc = s.scene.contents
    r = {"workload": "%s (Synth(%d)): %d views, %d polyline sets (%d polylines)" % (wl, CONFIG[wl], sc.n_views, n, len(ids)),
         "prior_cloud": {"points": cloud["n_points"], "intervals": int(rst["n_intervals"]),
                         "ms": {k: stats([x[k] for x in prior[1:]]) for k in prior[0]},
                         "replay_ms_graph": float(rst["ms_graph"]), "replay_ms_intervals": float(rst["ms_intervals"])},
         "stage_a": counts}
    names = {"a": "a_plain_call", "b": "b_null_manager", "c": "c_device_intervals"}
    for w in "abc":
        x = runs[w]
        r[names[w]] = {"points": x[0]["points"], "observations": x[0]["obs"], "tasks": x[0]["tasks"], "chains": x[0]["chains"],
                       "end_to_end_ms": stats([y["end_to_end"] for y in x]),
                       "stage_ms": {k: stats([y[k] for y in x]) for k in STAGES}}
    r["null_manager_equals_plain"] = all(runs["a"][0][k] == runs["b"][0][k] for k in ("points", "obs", "tasks", "chains"))
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
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "matched_sets.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
