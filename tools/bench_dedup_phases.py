#!/usr/bin/env python3
"""The dedup in phases against the combined call, and the merge of claim maps against a copy, on one GPU. One JSON line on
stdout and profiles/dedup_phases_<tag>.json (EG3D_BENCH_OUT overrides the path). Medians of `reps` (>= 10) with min and
max, by HIP events unless a figure says `wall` (perf_counter around the C-ABI call).

Per workload (C2 = Synth(2), C3' = Synth(3)), on the cloud a device-only match leaves in HBM:
  combined   eg3d_dedup_resident(no filter, no copy): its ms_dedup (events around k7_dedup_claim + k7_dedup_keep), and
             the wall time of eg3d_dedup_device;
  parent     the same two figures from ANOTHER build of the library (--parent-lib: libeg3d.so of the parent commit), measured
             by this script in a child process before this process opens the GPU;
  phased     eg3d_dedup_claim (offsets check + its read-back + claim), eg3d_dedup_keep, their sum — eg3d_dedup_phase_ms —
             and their wall times; the masks of the two forms are compared.
The merge (eg3d_dedup_merge_claims, k7_claims_min; eg3d_dedup_phase_ms = events around the kernel):
  c3 map     the real C3' maps: context A has claimed the first half of the cloud, B the second; "lowering" = A claims
             again, then merges B's map (some cells go down); "idle" = the same merge once more (none does);
  c4 size    a map of C4's n_cells (200 views x 534 x 400) on a small rig whose image is sized to give that many cells
             (a C4 context is not needed to move 171 MB): `other` claims a random 5 % of the cells of an empty map;
  each with the default form (a word is stored only if one of its cells was lowered) and with EG3D_MERGE_WRITE_ALL=1,
  next to hipMemcpyAsync device-to-device of the same bytes. The C ABI does not expose a context's stream: the copy runs on
  the null stream of an otherwise idle device, timed by events on that stream.

  python tools/bench_dedup_phases.py [reps=10] [--workloads c2,c3] [--parent-lib PATH] [--tag NAME]
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

ap = argparse.ArgumentParser(description="dedup in phases against the combined call; merge of claim maps against a copy")
ap.add_argument("reps", nargs="?", type=int, default=10)
ap.add_argument("--workloads", default="c2,c3")
ap.add_argument("--parent-lib", default=None, help="libeg3d.so of the parent commit")
ap.add_argument("--tag", default="mi355x")
ap.add_argument("--combined-only", action="store_true", help="(the child's mode) only the combined call, JSON on stdout")
opt = ap.parse_args()
reps = max(10, opt.reps)
CONFIG = {"c2": 2, "c3": 3}
workloads = [w for w in opt.workloads.split(",") if w]

parent = None
if opt.parent_lib and not opt.combined_only:   # before this process touches the GPU
    env = dict(os.environ, EG3D_LIB=os.path.abspath(opt.parent_lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(reps), "--workloads", opt.workloads, "--combined-only"],
                       env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit("the parent library's run failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    parent = json.loads(r.stdout.strip().splitlines()[-1])

from edgegraph3d_amd import _cdefs as D  # noqa: E402
from edgegraph3d_amd import api, host  # noqa: E402


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def wall(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def combined(ctx, dev, keep):
    ms, wl = [], []
    for i in range(reps + 2):
        _, _, st = ctx.dedup_resident(to_host=False)
        w, _ = wall(lambda: ctx.dedup_device(dev, keep=keep))
        if i >= 2:
            ms.append(st["ms_dedup"])
            wl.append(w)
    return {"ms_dedup": stats(ms), "dedup_device_wall": stats(wl)}


def open_workload(wl):
    s = host.Synth(CONFIG[wl])
    ctx = api.Context(s.scene)
    ctx.upload_seeds(s.seeds)
    ctx.match_resident(0, s.n_seeds, device_only=True)
    dev = ctx.last_device_output()
    return s, ctx, dev


if opt.combined_only:
    # (a build of the parent commit lacks the entry points of the newer tables: declare those of include/eg3d.h alone)
    from edgegraph3d_amd import _cabi
    api._LIB = _cabi.bind(C.CDLL(api.lib_path()), _cabi.EG3D)
    line = {}
    for wl in workloads:
        s, ctx, dev = open_workload(wl)
        line[wl] = combined(ctx, dev, ctx.device_alloc(int(dev.n_points)))
        ctx.close()
    print(json.dumps(line))
    sys.exit(0)

hip = api._hip()
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
EV = [C.c_void_p(), C.c_void_p()]
for e in EV:
    assert hip.hipEventCreate(C.byref(e)) == 0


def copy_ms(dst, src, nbytes):
    v = []
    for i in range(reps + 2):
        assert hip.hipEventRecord(EV[0], None) == 0
        assert hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), nbytes, 3, None) == 0
        assert hip.hipEventRecord(EV[1], None) == 0 and hip.hipEventSynchronize(EV[1]) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), EV[0], EV[1]) == 0
        if i >= 2:
            v.append(ms.value)
    return stats(v)


def with_store_form(always, make):
    """make() under EG3D_MERGE_WRITE_ALL (read once, when a context is created)."""
    if always:
        os.environ["EG3D_MERGE_WRITE_ALL"] = "1"
    try:
        return make()
    finally:
        os.environ.pop("EG3D_MERGE_WRITE_ALL", None)


line = {"reps": reps, "parent_lib": bool(parent)}
for wl in workloads:
    s, ctx, dev = open_workload(wl)
    sc = s.scene.contents
    n, m = int(dev.n_points), int(dev.n_obs)
    keep, keep2 = ctx.device_alloc(n), ctx.device_alloc(n)
    r = {"workload": "%s (Synth(%d)): %d seeds, %d views, %d points, %d observations" % (wl, CONFIG[wl], s.n_seeds, sc.n_views, n, m),
         "combined": combined(ctx, dev, keep)}
    if parent:
        r["parent_combined"] = parent[wl]
    cm, km, cw, kw = [], [], [], []
    for i in range(reps + 2):
        w1, _ = wall(lambda: ctx.dedup_claim(dev, 0, reset=True))
        t1 = ctx.dedup_phase_ms()
        w2, (_, n_kept) = wall(lambda: ctx.dedup_keep(dev, 0, keep2))
        t2 = ctx.dedup_phase_ms()
        if i >= 2:
            cm.append(t1), km.append(t2), cw.append(w1), kw.append(w2)
    ctx.dedup_device(dev, keep=keep)
    r["phased"] = {"claim_ms": stats(cm), "keep_ms": stats(km), "sum_ms": stats(np.add(cm, km)), "claim_wall": stats(cw),
                   "keep_wall": stats(kw), "sum_wall": stats(np.add(cw, kw)), "kept": n_kept,
                   "masks_identical": bool(np.array_equal(keep.numpy(np.uint8), keep2.numpy(np.uint8)))}
    base = r.get("parent_combined", r["combined"])
    r["phased_over_combined_ms"] = r["phased"]["sum_ms"]["median"] / base["ms_dedup"]["median"]
    r["phased_over_combined_wall"] = r["phased"]["sum_wall"]["median"] / base["dedup_device_wall"]["median"]
    if wl == "c3":   # the merge on the real maps: A = first half of the cloud, B = second half
        off = ctx.fetch_device_output()["obs_off"]
        half = n // 2
        first = D.DeviceEdgePoints()
        C.memmove(C.byref(first), C.byref(dev), C.sizeof(first))
        first.n_points, first.n_obs = half, int(off[half])
        second = D.DeviceEdgePoints()
        C.memmove(C.byref(second), C.byref(dev), C.sizeof(second))
        tail = ctx.upload(off[half:-1])
        second.n_points, second.obs_off = n - half, tail.ptr
        mg = {}
        for always in (False, True):
            A = with_store_form(always, lambda: api.Context(s.scene))   # (a clone would copy ctx's knobs)
            B = ctx.clone()
            B.dedup_claim(second, half, reset=True)
            pb, n_cells = B.dedup_claims()
            low, idle, n_low = [], [], 0
            for i in range(reps + 2):
                A.dedup_claim(first, 0, reset=True)
                n_low = A.dedup_merge_claims(pb, n_cells)
                t1 = A.dedup_phase_ms()
                assert A.dedup_merge_claims(pb, n_cells) == 0
                t2 = A.dedup_phase_ms()
                if i >= 2:
                    low.append(t1), idle.append(t2)
            mg["write_all" if always else "skip_store"] = {"lowering_ms": stats(low), "idle_ms": stats(idle), "n_lowered": n_low}
            pa, _ = A.dedup_claims()
            if not always:
                mg["n_cells"], mg["map_bytes"] = n_cells, 4 * n_cells
                mg["claimed_cells_A"] = int((A.fetch_dedup_claims() != 0xFFFFFFFF).sum())
                mg["copy_d2d_ms"] = copy_ms(pa, pb, 4 * n_cells)
            A.close(), B.close()
        r["merge_c3_maps"] = mg
    line[wl] = r
    ctx.close()
    s.close()

# ---- the merge at C4's map size ------------------------------------------------------------------------------------------------
V4 = host.default_config(4).n_views
small = host.Synth(0)
V0 = small.n_views
cells4 = V4 * 534 * 400                       # 200 views of 1600 x 1200
w = cells4 // (V0 * 400)
assert V0 * w * 400 == cells4
sc = D.Scene()
C.memmove(C.byref(sc), small.scene, C.sizeof(sc))
sc.width, sc.height = 3 * w, 1200
rng = np.random.default_rng(4)
other = np.full(cells4, 0xFFFFFFFF, np.uint32)
hit = rng.random(cells4) < 0.05
other[hit] = rng.integers(0, 2**31, int(hit.sum()), dtype=np.int64).astype(np.uint32)
mg = {"n_cells": cells4, "map_bytes": 4 * cells4, "claimed_share_of_other": 0.05}
for always in (False, True):
    A = with_store_form(always, lambda: api.Context(C.byref(sc)))
    d_other = A.upload(other)
    low, idle, n_low = [], [], 0
    for i in range(reps + 2):
        empty = D.DeviceEdgePoints()
        empty.complete = 1
        A.dedup_claim(empty, 0, reset=True)   # an empty cloud: the map is emptied, nothing is claimed
        n_low = A.dedup_merge_claims(d_other, cells4)
        t1 = A.dedup_phase_ms()
        assert A.dedup_merge_claims(d_other, cells4) == 0
        t2 = A.dedup_phase_ms()
        if i >= 2:
            low.append(t1), idle.append(t2)
    assert n_low == int(hit.sum())
    mg["write_all" if always else "skip_store"] = {"lowering_ms": stats(low), "idle_ms": stats(idle), "n_lowered": n_low}
    if not always:
        pa, n_cells = A.dedup_claims()
        assert n_cells == cells4
        mg["copy_d2d_ms"] = copy_ms(pa, d_other.ptr, 4 * cells4)
    d_other.free()
    A.close()
line["merge_c4_size"] = mg
for m_ in [line["merge_c4_size"]] + [line[w_]["merge_c3_maps"] for w_ in workloads if "merge_c3_maps" in line[w_]]:
    gb = 3 * m_["map_bytes"] / 1e9   # two maps read, one written at most
    m_["skip_store_lowering_TBps_of_3_maps"] = gb / m_["skip_store"]["lowering_ms"]["median"]
    m_["copy_TBps_of_2_maps"] = 2 * m_["map_bytes"] / 1e9 / m_["copy_d2d_ms"]["median"]
print(json.dumps(line))
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "dedup_phases_%s.json" % opt.tag)
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
