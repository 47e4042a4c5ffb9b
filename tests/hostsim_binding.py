"""ctypes binding of the test-only host simulation (tests/hostsim/libhostsim.so; libhostsim_dlt4x4.so is the same
compiled with the 4x4 form of the DLT system, rows = 2 of tests/forms.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from edgegraph3d_amd import _cdefs as D

_LIB = {}


def lib(rows=3):
    if rows not in _LIB:
        assert rows in (3, 2), rows
        d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
        subprocess.check_call(["make", "-s", "-j2", "-C", d])
        L = C.CDLL(os.path.join(d, "libhostsim.so" if rows == 3 else "libhostsim_dlt4x4.so"))
        L.hostsim_match.argtypes = [C.POINTER(D.Scene), C.POINTER(D.Seeds), C.c_uint32, C.c_uint32,
                                    C.POINTER(D.Candidates), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                    C.POINTER(D.EdgePoints)]
        L.hostsim_free_edgepoints.argtypes = [C.POINTER(D.EdgePoints)]
        L.hostsim_reach.argtypes = [C.c_int, C.POINTER(C.c_ulonglong), C.c_int]
        L.hostsim_closest_pruned_mismatches.argtypes = [D.f32p, C.c_int, D.f32p, C.c_int, C.c_uint32, C.c_uint32]
        L.hostsim_walk_pf_mismatches.argtypes = [D.f32p, C.c_int, C.c_uint32, C.c_uint32, D.f32p, C.c_int]
        L.hostsim_dist2.restype = C.c_float
        L.hostsim_dist2.argtypes = [C.c_float] * 4
        L.hostsim_seg_closest.restype = C.c_float
        L.hostsim_seg_closest.argtypes = [C.c_float] * 6 + [D.f32p]
        L.hostsim_walk_by_distance.argtypes = [D.f32p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                                               C.c_float, C.c_uint32, C.c_float, D.u32p, D.f32p]
        L.hostsim_walk_by_line.argtypes = [D.f32p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float,
                                           C.c_uint32, D.f32p, C.c_int, C.c_float, C.c_float, D.u32p, D.f32p]
        L.hostsim_triangulate.argtypes = [D.f32p, D.i32p, D.f32p, C.c_int, D.f32p]
        L.hostsim_gn_filter.argtypes = [D.f32p, D.f32p, D.u32p, D.i32p, D.f32p, C.c_uint64, C.c_float, C.c_int,
                                        D.f32p, D.u8p]
        _LIB[rows] = L
    return _LIB[rows]


def match(scene_ptr, seeds_ptr, begin, end, cand_struct, hyp_cap=192, chain_cap=768, pool_cap=8192, slot_step=False, rows=3):
    e = D.EdgePoints()
    rc = lib(rows).hostsim_match(scene_ptr, seeds_ptr, begin, end, C.byref(cand_struct), hyp_cap, chain_cap, pool_cap,
                             int(slot_step), C.byref(e))
    if rc != 0:
        raise RuntimeError("hostsim_match rc=%d" % rc)
    d = D.edgepoints_to_dict(e)
    lib(rows).hostsim_free_edgepoints(C.byref(e))
    return d


REACH_BINS = 4096
REACH_SIDE_WALK, REACH_SOLVE_ROWS, REACH_STEP_FIRST, REACH_STEP_LATER = range(4)


def reach(what, rows=3):
    """Histogram `what` (REACH_*) of the last match() of that form: {value: events}. The counters sit in the sequential statement of the
    expand stage (EG3D_REACH in eg3d_dev_expand.h, nothing on the device): lines one side walk consumed, rows of one solve
    with the extra row of an ADD request, list length of an N-view step when its first / a later starting observation is
    walked."""
    h = np.zeros(REACH_BINS, np.uint64)
    rc = lib(rows).hostsim_reach(what, h.ctypes.data_as(C.POINTER(C.c_ulonglong)), REACH_BINS)
    if rc < 0:
        raise RuntimeError("hostsim_reach rc=%d" % rc)
    assert h[-1] == 0, "a reach value of %d or more: enlarge HOSTSIM_REACH_BINS" % (REACH_BINS - 1)
    return {int(v): int(h[v]) for v in np.nonzero(h)[0]}
