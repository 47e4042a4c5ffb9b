#!/usr/bin/env python3
"""Pipelines 1-2 with the polyline sets resident on the device (include/eg3d_sets_device.h), on one GPU. One JSON line on
stdout and profiles/sets_device.json (EG3D_BENCH_OUT overrides the path). No figure here is a pass condition except the
last: the existing call must cost what it cost on the parent commit.

Per workload (C2 = Synth(2), C3' = Synth(3)) one child process under its own time limit (a fault or a hang of one workload
ends that child, and nothing is started after it). Inside it:
  k13        eg3d_similarity_graph and eg3d_detect_communities once, then `reps` repetitions each of K13 on the ids K11 left
             on the device (its own ms_device and the call's wall time) and of what it replaces: eg3d_host_sets_from_communities
             plus eg3d_upload_polyline_sets of its rows.
  pipeline1  C2 ONLY, K11's communities: eg3d_match_polyline_sets on the host rows against eg3d_match_polyline_items on the
             resident sets, on 1 and 3 lanes, each with the copy of its cloud, alternating; the units each forms (the items
             call reports its own; the sets call's are derived from its rule: runs of whole sets within max_items, at least
             one per lane). C3''s six communities are NOT run: nobody has measured what that input costs.
  existing   the workload's curve sets through eg3d_match_polyline_sets of THIS build and of the parent's (--parent-lib, a
             libeg3d.so built from the parent commit), one context each, alternating, `reps` repetitions: both
             distributions, and whether this build's median lies inside the parent's own spread.

  python tools/bench_sets_device.py [reps=10] [--workloads c2,c3] [--parent-lib PATH] [--limit SECONDS]
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

ap = argparse.ArgumentParser(description="resident polyline sets: K13, the items call, the existing call against the parent")
ap.add_argument("reps", nargs="?", type=int, default=10, help="repetitions of each path (at least 10)")
ap.add_argument("--workloads", default="c2,c3", help="comma-separated: c2, c3")
ap.add_argument("--parent-lib", default=None, help="libeg3d.so of the parent commit (the `existing` section needs it)")
ap.add_argument("--limit", type=int, default=400, help="time limit of one workload's child process, seconds")
ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
opt = ap.parse_args()
reps = max(10, opt.reps)
CONFIG = {"c2": 2, "c3": 3}


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def worker(wl):
    from edgegraph3d_amd import _cabi
    from edgegraph3d_amd import _cdefs as D
    from edgegraph3d_amd import api, host
    L = api.lib()
    s = host.Synth(CONFIG[wl])
    ctx = api.Context(s.scene)
    V = ctx.n_views
    r = {}

    # ---- K13 against the host statement + the upload it replaces
    g = ctx.similarity_graph(s.seeds)
    com = ctx.communities(g)
    n = int(g["n_nodes"])
    k13_dev, k13_wall, host_ms, up_ms = [], [], [], []
    for i in range(reps + 2):
        t0 = time.perf_counter()
        view, st = ctx.sets_from_communities_device(None, n=n, with_stats=True)
        t1 = time.perf_counter()
        rows = host.sets_from_communities(g, com["ids"], V)
        t2 = time.perf_counter()
        ctx.upload_polyline_sets(*rows)
        t3 = time.perf_counter()
        if i >= 2:
            k13_dev.append(st["ms_device"])
            k13_wall.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
            up_ms.append((t3 - t2) * 1e3)
    r["k13"] = {"nodes": n, "communities": int(com["n_communities"]), "sets": rows[0], "ids": int(len(rows[2])),
                "k13_ms_device": stats(k13_dev), "k13_call_ms": stats(k13_wall),
                "host_sets_from_communities_ms": stats(host_ms), "upload_and_check_ms": stats(up_ms)}

    # ---- pipeline 1 on K11's communities (C2 only)
    if wl == "c2":
        n_sets, row_off, ids = rows
        view = ctx.sets_from_communities_device(None, n=n)
        max_items = 2048 if V >= 64 else 16384
        p1 = {"communities": n_sets, "items": int(len(ids))}
        for lanes in (1, 3):
            ctx.set_pipelining(lanes, 0)
            a, b, units = [], [], None
            for i in range(reps + 2):
                t0 = time.perf_counter()
                x = ctx.match_polyline_sets(n_sets, row_off, ids)
                t1 = time.perf_counter()
                y = ctx.match_polyline_items(view)
                t2 = time.perf_counter()
                assert x["n_points"] == y["n_points"] and x["n_obs"] == y["n_obs"]
                units = y["n_units"]
                if i >= 2:
                    a.append((t1 - t0) * 1e3)
                    b.append((t2 - t1) * 1e3)
            whole_sets_units = max(min(lanes, n_sets), -(-int(len(ids)) // max_items))   # (every community fits max_items here)
            p1["lanes_%d" % lanes] = {"points": x["n_points"], "samples": x["n_tasks"],
                                      "match_polyline_sets_ms": stats(a), "match_polyline_items_ms": stats(b),
                                      "units_sets_call_by_its_rule": whole_sets_units, "units_items_call": units}
        r["pipeline1"] = p1
        ctx.set_pipelining(0, 0)

    # ---- the existing call, this build against the parent's, interleaved
    if opt.parent_lib:
        Lp = _cabi.bind(C.CDLL(os.path.abspath(opt.parent_lib)), _cabi.EG3D)
        n_sets, row_off, ids = s.polyline_sets()
        row_off = np.ascontiguousarray(row_off, np.uint32)
        ids = np.ascontiguousarray(ids if len(ids) else [0], np.uint32)
        ps = D.PolylineSets(n_sets, D.np_ptr(row_off, C.c_uint32), D.np_ptr(ids, C.c_uint32))
        hp = C.c_void_p()
        assert Lp.eg3d_create(s.scene, 0, C.byref(hp)) == 0, Lp.eg3d_last_error()

        def call(lib, h):
            e, tm = D.EdgePoints(), D.StageTimes()
            t0 = time.perf_counter()
            rc = lib.eg3d_match_polyline_sets(h, C.byref(ps), 0, n_sets, 0, C.byref(e), C.byref(tm))
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, lib.eg3d_last_error()
            pts = int(e.n_points)
            lib.eg3d_free_edgepoints(C.byref(e))
            return dt, pts

        both = {"parent": (Lp, hp), "this": (L, ctx._h)}
        t = {k: [] for k in both}
        for i in range(reps + 2):
            for k, (lib, h) in both.items():
                dt, pts = call(lib, h)
                if i >= 2:
                    t[k].append(dt)
        Lp.eg3d_destroy(hp)
        sp, st_ = stats(t["parent"]), stats(t["this"])
        r["existing"] = {"sets": n_sets, "points": pts, "parent_ms": sp, "this_ms": st_, "parent_all": t["parent"], "this_all": t["this"],
                         "this_median_inside_parent_spread": bool(sp["min"] <= st_["median"] <= sp["max"] or st_["median"] <= sp["min"])}
    ctx.close()
    s.close()
    print("RESULT " + json.dumps(r), flush=True)


if opt.worker:
    worker(opt.worker)
    sys.exit(0)

line = {"reps": reps}
for wl in [w for w in opt.workloads.split(",") if w]:
    cmd = ["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), str(reps), "--worker", wl]
    if opt.parent_lib:
        cmd += ["--parent-lib", opt.parent_lib]
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
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "sets_device.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
