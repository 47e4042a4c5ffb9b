#!/usr/bin/env python3
"""The filter stage on a device-resident cloud against the path through the host, on one GPU. One JSON line on stdout
and profiles/filter_resident_c3.json (EG3D_BENCH_OUT overrides the path).

 (a) C3' (Synth(3)), one process, warm-up, `reps` repetitions of each, interleaved:
       host path:     eg3d_match_resident to the host -> eg3d_gn_filter from the host arrays (offsets narrowed to 32 bits)
                      -> threshold (eg3d_host_observation_filter) -> numpy compaction of the seven arrays
       resident path: device-only match -> eg3d_filter_resident(to_host = 1)
     both timed at the C ABI (no conversion of the match output to numpy), survivors compared bit for bit once.
 (b) kernel time (HIP events) of k5_gn_filter<uint64_t, no sentinel> against k5_gn_filter<uint32_t, sentinel> on the
     config-5 input of tools/bench_gn_filter.py (1 M points), interleaved launches.
 (c) ms_compact of (a) beside the bytes the three launches move, as a share of the HBM peak; and the same with
     non-temporal loads of the source (EG3D_COMPACT_NT=1 on a second context).

  python tools/bench_filter_resident.py [reps=10] [n_points_b=1000000]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgegraph3d_amd import _cdefs as D  # noqa: E402
from edgegraph3d_amd import api, host  # noqa: E402
from edgegraph3d_amd.cloudnp import np_compact, same_cloud  # noqa: E402

_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(_pos[0]) if len(_pos) > 0 else 10
n_b = int(_pos[1]) if len(_pos) > 1 else 1000000
MSE = 2.25
HBM_PEAK_GBPS = 8000.0   # spec
HBM_COPY_GBPS = 6300.0   # what a float4 copy kernel reaches on this part
L, H = api.lib(), host.lib()


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def host_path(ctx, n_seeds, V, keep_result=False):
    t = [time.perf_counter()]
    e, tm = D.EdgePoints(), D.StageTimes()
    assert L.eg3d_match_resident(ctx._h, 0, n_seeds, 0, C.byref(e), C.byref(tm)) == 0
    t.append(time.perf_counter())
    n, m = int(e.n_points), int(e.n_obs)
    off64 = np.ctypeslib.as_array(e.obs_off, shape=(n + 1,))
    off32 = off64.astype(np.uint32)                      # the host entry point takes 32-bit offsets
    Xo, inl, ms = np.empty((n, 3), np.float32), np.empty(n, np.uint8), C.c_float(0)
    assert L.eg3d_gn_filter(ctx._h, e.X, D.np_ptr(off32, C.c_uint32), e.obs_view, e.obs_xy, n, MSE, 0, D.np_ptr(Xo, C.c_float),
                            D.np_ptr(inl, C.c_uint8), C.byref(ms)) == 0
    t.append(time.perf_counter())
    thr = H.eg3d_host_observation_filter(V, D.np_ptr(off32, C.c_uint32), n, 0, -1, D.np_ptr(inl, C.c_uint8))
    cloud = {"X": np.ctypeslib.as_array(e.X, shape=(n, 3)), "obs_off": off64, "key": np.ctypeslib.as_array(e.key, shape=(n, 4)),
             "obs_view": np.ctypeslib.as_array(e.obs_view, shape=(m,)), "obs_pl": np.ctypeslib.as_array(e.obs_pl, shape=(m,)),
             "obs_seg": np.ctypeslib.as_array(e.obs_seg, shape=(m,)), "obs_xy": np.ctypeslib.as_array(e.obs_xy, shape=(m, 2))}
    out = np_compact(cloud, inl, Xo)
    t.append(time.perf_counter())
    L.eg3d_free_edgepoints(C.byref(e))
    d = np.diff(t) * 1e3
    return {"total": float(d.sum()), "match_to_host": float(d[0]), "gn_filter_host_arrays": float(d[1]),
            "threshold_and_numpy_compaction": float(d[2]), "kernel": ms.value, "n": n, "m": m, "threshold": thr,
            "result": out if keep_result else None, "kept": (out["n_points"], out["n_obs"])}


def resident_path(ctx, n_seeds, keep_result=False):
    t0 = time.perf_counter()
    e, tm = D.EdgePoints(), D.StageTimes()
    assert L.eg3d_match_resident(ctx._h, 0, n_seeds, 1, C.byref(e), C.byref(tm)) == 0
    t1 = time.perf_counter()
    o, st = D.EdgePoints(), D.FilterStats()
    st.struct_size = C.sizeof(D.FilterStats)
    assert L.eg3d_filter_resident(ctx._h, MSE, 0, -1, None, 1, C.byref(o), None, C.byref(st)) == 0
    t2 = time.perf_counter()
    res = D.edgepoints_to_dict(o) if keep_result else None
    L.eg3d_free_edgepoints(C.byref(o))
    return {"total": (t2 - t0) * 1e3, "match_device_only": (t1 - t0) * 1e3, "filter_resident": (t2 - t1) * 1e3,
            "ms_filter": st.ms_filter, "ms_compact": st.ms_compact, "ms_copy": st.ms_copy, "threshold": st.threshold,
            "kept": (int(st.n_kept), int(st.n_obs_kept)), "n": int(st.n_points_in), "result": res}


def compact_bytes(n, m, np_, no):
    # count pass: offsets + mask; scatter: offsets + mask again, X and key of the survivors, 20 B per surviving observation,
    # and the survivors written (36 B per point, 20 B per observation); block totals are noise
    return 2 * n * 9 + np_ * (12 + 16) + no * 20 + np_ * 36 + no * 20


line = {"reps": reps, "gn_max_mse": MSE}
# ---------------------------------------------------------------- (a)
s = host.Synth(3)
V = s.n_views
ctx = api.Context(s.scene)
ctx.upload_seeds(s.seeds)
ns = s.n_seeds
a0, b0 = host_path(ctx, ns, V, True), resident_path(ctx, ns, True)     # warm-up (and the comparison)
same = same_cloud(a0["result"], b0["result"]) is None and a0["threshold"] == b0["threshold"]
host_path(ctx, ns, V), resident_path(ctx, ns)                            # second warm-up: pipelining lanes of the host call exist now
ha, rb = [], []
for _ in range(reps):
    ha.append(host_path(ctx, ns, V))
    rb.append(resident_path(ctx, ns))
n, m = a0["n"], a0["m"]
np_, no = a0["kept"]
a = {"workload": "C3' (Synth(3)): %d seeds, %d points, %d observations; %d points / %d observations kept (threshold %d)"
                 % (ns, n, m, np_, no, a0["threshold"]),
     "results_bit_identical": bool(same),
     "host_path_ms": {k: stats([r[k] for r in ha]) for k in ("total", "match_to_host", "gn_filter_host_arrays",
                                                             "threshold_and_numpy_compaction", "kernel")},
     "resident_path_ms": {k: stats([r[k] for r in rb]) for k in ("total", "match_device_only", "filter_resident", "ms_filter",
                                                                "ms_compact", "ms_copy")},
     "host_path_bytes": {"d2h": 36 * n + 8 + 20 * m + 13 * n, "h2d": 12 * n + 4 * (n + 1) + 12 * m},
     "resident_path_bytes": {"d2h": 36 * np_ + 20 * no + 8 * (V + 3) + 24, "h2d": 0}}
a["speedup_total"] = a["host_path_ms"]["total"]["median"] / a["resident_path_ms"]["total"]["median"]
a["speedup_filter_stage"] = ((a["host_path_ms"]["total"]["median"] - a["resident_path_ms"]["match_device_only"]["median"])
                             / a["resident_path_ms"]["filter_resident"]["median"])
line["a_c3_host_vs_resident"] = a
# ---------------------------------------------------------------- (c)
cb = compact_bytes(n, m, np_, no)
mc = a["resident_path_ms"]["ms_compact"]
ctx_nt = None
os.environ["EG3D_COMPACT_NT"] = "1"
ctx_nt = api.Context(s.scene)
del os.environ["EG3D_COMPACT_NT"]
ctx_nt.upload_seeds(s.seeds)
resident_path(ctx_nt, ns)
pl, nt = [], []
for _ in range(reps):
    pl.append(resident_path(ctx, ns)["ms_compact"])
    nt.append(resident_path(ctx_nt, ns)["ms_compact"])
ctx_nt.close()
line["c_compaction"] = {"bytes_moved": cb, "ms_compact": mc, "GBps": cb / (mc["median"] * 1e-3) / 1e9,
                        "frac_of_hbm_peak": cb / (mc["median"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, "hbm_peak_GBps": HBM_PEAK_GBPS,
                        "frac_of_achievable_copy": cb / (mc["median"] * 1e-3) / 1e9 / HBM_COPY_GBPS, "achievable_copy_GBps": HBM_COPY_GBPS,
                        "note": "ms_compact spans three launches AND the host read-back of the totals between the scan and the "
                                "scatter (the output buffers are sized from it)",
                        "interleaved_plain_loads_ms": stats(pl), "interleaved_nontemporal_loads_ms": stats(nt)}
ctx.close()
# ---------------------------------------------------------------- (b)
s5 = host.Synth(5)
X, off, view, xy = s5.points(n_b)
c5 = api.Context(s5.scene)
dev = D.DeviceEdgePoints()
keepalive = [c5.upload(X), c5.upload(off[:-1].astype(np.uint64)), c5.upload(view), c5.upload(xy)]
dev.n_points, dev.n_obs, dev.complete = n_b, int(off[-1]), 1
dev.X, dev.obs_off, dev.obs_view, dev.obs_xy = [k.ptr for k in keepalive]
Xd, inld = c5.device_alloc(12 * n_b), c5.device_alloc(n_b)
old_ms, new_ms = [], []
for i in range(reps + 1):
    Xo, inl, mo = c5.gn_filter(X, off, view, xy, MSE)
    _, _, hist, _, mn = c5.gn_filter_device(dev, None, MSE, False, X_out=Xd, inlier=inld)
    if i:
        old_ms.append(mo)
        new_ms.append(mn)
same_b = bool(np.array_equal(inld.numpy(np.uint8), inl) and np.array_equal(Xd.numpy(np.uint32), Xo.view(np.uint32).ravel()))
line["b_kernel_c5"] = {"workload": "C5 synthetic: %d points, %d observations" % (n_b, int(off[-1])),
                       "k5_gn_filter_u32_sentinel_ms": stats(old_ms), "k5_gn_filter_u64_device_ms": stats(new_ms),
                       "ratio_median": float(np.median(new_ms) / np.median(old_ms)), "results_bit_identical": same_b}
c5.close()
print(json.dumps(line))
out = os.environ.get("EG3D_BENCH_OUT") or os.path.join(ROOT, "profiles", "filter_resident_c3.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
