"""The cooperative form of walk_by_line (eg3d_dev_geom.h: walk_by_line_head + walk_seg_test + walk_resolve — what the K3a
engine's walk service runs, eg3d_k3a_engine.h) against walk_by_line itself, on the host: tests/walkcoop/walkcoop.cpp
emulates the 64 lanes of a pass with a loop. Compared: the return code, the segment, the bits of x and y (what the
walk leaves untouched is compared too: both start from the same sentinel). Required: zero mismatches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (2, 3, 5, 6, 64, 65, 66, 129, 300)
HEADS = (1, 2, 3, 4)
f32p = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def wc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("walkcoop") / "libwalkcoop.so")
    # the arithmetic contract of the product's host code (edgegraph3d_amd/build.py HOST_FLAGS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                           "-I", os.path.join(ROOT, "edgegraph3d_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "walkcoop", "walkcoop.cpp")])
    L = C.CDLL(so)
    L.walkcoop_sweep.argtypes = [C.c_int, f32p, C.c_uint32] + [C.c_float] * 6 + [u32p] * 3
    L.walkcoop_sweep.restype = C.c_int
    return L


class Tally:
    def __init__(self):
        self.cases = C.c_uint32(0)
        self.long = C.c_uint32(0)
        self.multi = C.c_uint32(0)


def sweep(L, T, v, frac, line, tally, min_d=5.0, max_d=15.0):
    """every start segment x {towards start, towards end, neither} x {unbounded, bounded}; returns the mismatches"""
    v = np.ascontiguousarray(v, np.float32)
    la, lb, lc = (np.float32(t) for t in line)
    bad = L.walkcoop_sweep(T, v.ctypes.data_as(f32p), len(v), frac, la, lb, lc, min_d, max_d, C.byref(tally.cases),
                           C.byref(tally.long), C.byref(tally.multi))
    assert bad >= 0
    return bad


def polyline(rng, n):
    """a wandering pixel chain: steps of 2-6 px with a slowly turning heading"""
    head = rng.uniform(0, 2 * np.pi) + np.cumsum(rng.normal(0, 0.35, n))
    step = rng.uniform(2.0, 6.0, n)
    xy = np.cumsum(np.stack([np.cos(head) * step, np.sin(head) * step], 1), 0) + rng.uniform(100, 900, 2)
    return xy.astype(np.float32)


def line_through(p, ang):
    """a x + b y + c = 0 through p with direction angle ang"""
    a, b = np.float32(-np.sin(ang)), np.float32(np.cos(ang))
    return a, b, np.float32(-(np.float64(a) * p[0] + np.float64(b) * p[1]))


@pytest.mark.parametrize("T", HEADS)
def test_random_polylines_and_lines(wc, T):
    rng = np.random.default_rng(100 + T)
    tally, bad = Tally(), 0
    for n in SIZES:
        for _ in range(6):
            v = polyline(rng, n)
            for _ in range(6):
                # lines that cross the polyline somewhere, and lines that miss it (walks to the extreme)
                p = v[rng.integers(0, n)] + rng.normal(0, 1, 2) * (0.5 if rng.random() < 0.7 else 400.0)
                bad += sweep(wc, T, v, np.float32(rng.uniform(0, 1)), line_through(p, rng.uniform(0, np.pi)), tally)
    assert bad == 0
    assert tally.long.value > 0 and tally.multi.value > 0  # walks past the head, and of several passes (129, 300 vertices)


@pytest.mark.parametrize("T", HEADS)
def test_line_through_a_vertex_and_axis_lines(wc, T):
    rng = np.random.default_rng(200 + T)
    tally, bad = Tally(), 0
    for n in SIZES:
        v = np.round(polyline(rng, n))  # integer vertices: t = 0 and t = 1 are hit exactly
        for i in sorted({0, 1, n // 2, n - 2, n - 1}):
            x, y = float(v[i][0]), float(v[i][1])
            for line in ((1.0, 0.0, -x), (0.0, 1.0, -y), (1.0, 1.0, -(x + y)), (1.0, -1.0, -(x - y))):  # (b = 0: the vertical case of line_dir)
                for frac in (0.0, 0.5, 1.0):
                    bad += sweep(wc, T, v, frac, line, tally)
    assert bad == 0 and tally.long.value > 0


@pytest.mark.parametrize("T", HEADS)
def test_quasi_parallel_stop(wc, T):
    """a line within 5 px of a segment and parallel to it (or nearly): the walk stops there, wherever the segment lies
    — in the head, in the first pass, in a later pass"""
    rng = np.random.default_rng(300 + T)
    tally, bad = Tally(), 0
    for n in SIZES:
        v = polyline(rng, n)
        for i in sorted({0, min(2, n - 2), min(5, n - 2), min(70, n - 2), n - 2}):
            d = (v[i + 1] - v[i]).astype(np.float64)
            ang = np.arctan2(d[1], d[0])
            nrm = np.array([-np.sin(ang), np.cos(ang)])
            for off in (0.0, 2.0, 4.9, 5.1, 30.0):
                for tilt in (0.0, 0.05, 0.3):
                    line = line_through(v[i].astype(np.float64) + nrm * off, ang + tilt)
                    bad += sweep(wc, T, v, np.float32(0.25), line, tally)
    assert bad == 0 and tally.long.value > 0


@pytest.mark.parametrize("T", HEADS)
def test_zero_length_segments_nan_lines_and_windows(wc, T):
    rng = np.random.default_rng(400 + T)
    tally, bad = Tally(), 0
    nan, inf = float("nan"), float("inf")
    for n in SIZES:
        v = polyline(rng, n)
        rep = v.copy()
        for i in range(1, n, 3):  # repeated vertices: zero-length segments (den == 0: the distance branch)
            rep[i] = rep[i - 1]
        for w in (v, rep, np.repeat(v[:1], n, 0)):
            p = w[n // 2]
            for line in (line_through(p, 0.7), (nan, 1.0, 0.0), (1.0, nan, 0.0), (1.0, 1.0, nan), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0),
                         (inf, 1.0, 0.0), (1e-30, 1e-30, 0.0), (1e30, -1e30, 1.0)):
                bad += sweep(wc, T, w, np.float32(0.5), line, tally)
            # the [min, max] window on both sides of a hit: accepted, too near, too far, empty, NaN
            for mn, mx in ((0.0, 1e9), (5.0, 15.0), (0.0, 0.5), (50.0, 60.0), (10.0, 5.0), (nan, nan)):
                bad += sweep(wc, T, w, np.float32(0.5), line_through(w[min(n - 1, n // 2 + 3)], 1.1), tally, mn, mx)
    assert bad == 0 and tally.cases.value > 0
