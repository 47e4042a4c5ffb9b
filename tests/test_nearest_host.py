"""The sequential statement of the cloud-to-cloud nearest distances (include/eg3d/host_nearest.hpp, libeg3d_host.so) without a
GPU: eg3d_host_cloud_nearest against the independent numpy brute force of tests/nearest_ref.py on every case of
tests/nearest_cases.py — all d2 bits, all nn, every figure —, its refusals, each with its own code and with the outputs
untouched, the figures of its grid, and the PLY point reader on files written here."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import nearest_cases as nc
import nearest_ref
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import host

F = np.float32


def host_result(case):
    return host.cloud_nearest(case["ref"], case["X"], case["max_dist"], cell=case["cell"], ref_keep=case["ref_keep"], keep=case["keep"],
                              thresholds=case["thresholds"])


# ---- the statement against the brute force -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nc.CASES, ids=nc.IDS)
def test_host_statement_is_the_brute_force(case):
    nc.assert_same(host_result(case), nc.reference(case), case["name"])


@pytest.mark.parametrize("case", nc.CASES, ids=nc.IDS)
def test_host_grid_figures(case):
    got, want = host.cloud_index_stats(case["ref"], case["cell"], case["ref_keep"]), nearest_ref.index_figures(case["ref"], case["cell"], case["ref_keep"])
    for f in ("n_points", "n_dropped", "n_nonfinite", "n_indexed", "n_cells", "max_cell_points", "dims"):
        assert got[f] == want[f], (f, got[f], want[f])
    assert np.array_equal(got["origin"], want["origin"])


def test_the_cases_exercise_what_they_name():
    by = {c["name"]: c for c in nc.CASES}
    # exactly at max_dist: excluded; one ulp nearer: included (the first 6 x 2 boundary queries, per axis and sign)
    for name in ("boundary_single_md0.25", "boundary_single_md0.3"):
        d2, nn, fig = nc.reference(by[name])
        for q in range(0, 12, 2):
            assert nn[q] == nearest_ref.NONE and np.isinf(d2[q])
            assert nn[q + 1] == 0 and d2[q + 1] < F(F(by[name]["max_dist"]) * F(by[name]["max_dist"]))
        assert fig["n_below"][0] == fig["n_within"]    # (a threshold equal to max_dist counts the whole within set)
    # ties: the smaller index of duplicates and of two equidistant references
    d2, nn, _ = nc.reference(by["ties"])
    assert list(nn[:4]) == [0, 0, 1, 4] and d2[0] == F(0.0625)
    # the crowded cell, the empty reference, non-finite and dropped counts
    assert nearest_ref.index_figures(by["crowded_cell"]["ref"], 0.5)["max_cell_points"] >= 1000
    assert nc.reference(by["n_ref_0"])[2]["n_within"] == 0 and np.isinf(nc.reference(by["n_ref_0"])[2]["median_d2"])
    assert nc.reference(by["nonfinite"])[2]["n_nonfinite"] == 4 and nearest_ref.index_figures(by["nonfinite"]["ref"], 0.25)["n_nonfinite"] == 4
    k = nc.reference(by["keep_masks"])[2]
    assert k["n_dropped"] > 0 and k["n_nonfinite"] > 0 and k["n_within"] > 0
    assert len(by["md_far_below_cell"]["thresholds"]) == 8 and by["md_far_below_cell"]["thresholds"][0] == by["md_far_below_cell"]["max_dist"]
    r = nc.reference(by["random_3000x2000"])[2]
    assert r["n_queries"] == 3000 and 0 < r["n_within"] < 3000
    # far queries and queries just outside the box find nothing / something
    o = nc.reference(by["outside_box"])
    assert (o[1][-3:] == nearest_ref.NONE).all()
    assert (o[1][0:12:2] != nearest_ref.NONE).all() and (o[1][1:12:2] == nearest_ref.NONE).all()


def test_mean_and_median_are_distances():
    c = nc.CASES[nc.IDS.index("random_3000x2000")]
    d2, nn, st = host_result(c)
    within = nn != nearest_ref.NONE
    dist = np.sqrt(d2[within].astype(np.float64))
    assert abs(st["mean"] - dist.mean()) <= c["max_dist"] * 2.0 ** -32 + 1e-15    # each term is floored to max_dist * 2^-32
    assert st["mean"] <= dist.mean()
    assert st["median"] == np.sqrt(np.float64(np.sort(d2[within])[(within.sum() - 1) // 2]))


def test_null_outputs_and_no_stats():
    c = nc.CASES[nc.IDS.index("one_cell")]
    L = host.lib()
    R, Q = c["ref"], c["X"]
    st = D.nearest_stats_new(c["thresholds"])
    rc = L.eg3d_host_cloud_nearest(D.np_ptr(R, C.c_float), len(R), None, D.np_ptr(Q, C.c_float), len(Q), None, c["cell"], c["max_dist"],
                                   None, None, C.byref(st))
    assert rc == 0
    want = nc.reference(c)[2]
    got = D.nearest_stats_to_dict(st, c["max_dist"])
    for f in nc.FIGURES:
        assert got[f] == want[f], f
    d2 = np.empty(len(Q), F)
    assert L.eg3d_host_cloud_nearest(D.np_ptr(R, C.c_float), len(R), None, D.np_ptr(Q, C.c_float), len(Q), None, c["cell"], c["max_dist"],
                                     D.np_ptr(d2, C.c_float), None, None) == 0
    assert np.array_equal(d2.view(np.uint32), nc.reference(c)[0].view(np.uint32))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
R3 = np.array([[0, 0, 0], [1, 1, 1]], F)
REFUSALS = [
    ("cell_zero", dict(cell=0.0, max_dist=0.1), host.NEAREST_ERR_CELL),
    ("cell_negative", dict(cell=-1.0, max_dist=0.1), host.NEAREST_ERR_CELL),
    ("cell_nan", dict(cell=float("nan"), max_dist=0.1), host.NEAREST_ERR_CELL),
    ("cell_inf", dict(cell=float("inf"), max_dist=0.1), host.NEAREST_ERR_CELL),
    ("max_dist_zero", dict(cell=1.0, max_dist=0.0), host.NEAREST_ERR_MAXDIST),
    ("max_dist_nan", dict(cell=1.0, max_dist=float("nan")), host.NEAREST_ERR_MAXDIST),
    ("max_dist_above_cell", dict(cell=0.5, max_dist=0.5000001), host.NEAREST_ERR_MAXDIST),
    ("nine_thresholds", dict(cell=1.0, max_dist=0.5, thresholds=(0.1,) * 9), host.NEAREST_ERR_THRESHOLD),
    ("threshold_above_max_dist", dict(cell=1.0, max_dist=0.5, thresholds=(0.1, 0.6)), host.NEAREST_ERR_THRESHOLD),
    ("threshold_zero", dict(cell=1.0, max_dist=0.5, thresholds=(0.0,)), host.NEAREST_ERR_THRESHOLD),
    ("threshold_nan", dict(cell=1.0, max_dist=0.5, thresholds=(float("nan"),)), host.NEAREST_ERR_THRESHOLD),
    ("extent", dict(cell=1.0, max_dist=0.5, ref=np.array([[0, 0, 0], [0, 2097151.5, 0]], F)), host.NEAREST_ERR_EXTENT),
]


@pytest.mark.parametrize("name,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_have_their_codes_and_leave_the_outputs_untouched(name, kw, code):
    kw = dict(kw)
    ref = kw.pop("ref", R3)
    d2, nn = np.full(3, 7.5, F), np.full(3, 12345, np.uint32)
    with pytest.raises(host.NearestError) as e:
        host.cloud_nearest(ref, np.zeros((3, 3), F), d2=d2, nn=nn, **kw)
    assert e.value.code == code and "eg3d_host_cloud_nearest" in str(e.value)
    assert (d2 == 7.5).all() and (nn == 12345).all()


def test_the_largest_extent_that_is_accepted():
    ref = np.array([[0, 0, 0], [0, 2097150.5, 0]], F)    # 2^21 - 1 cells on y
    assert host.cloud_index_stats(ref, 1.0)["dims"] == [1, 2097151, 1]
    d2, nn, st = host.cloud_nearest(ref, ref, 0.5, cell=1.0)
    assert list(nn) == [0, 1] and st["n_within"] == 2


def test_struct_size_and_null_arrays_are_refused():
    L = host.lib()
    small = D.NearestStats(struct_size=8)
    q = np.zeros(3, F)
    assert L.eg3d_host_cloud_nearest(D.np_ptr(q, C.c_float), 1, None, D.np_ptr(q, C.c_float), 1, None, 1.0, 0.5, None, None, C.byref(small)) == -1
    assert b"struct_size" in L.eg3d_host_nearest_last_error() and small.n_queries == 0
    assert L.eg3d_host_cloud_nearest(None, 1, None, D.np_ptr(q, C.c_float), 1, None, 1.0, 0.5, None, None, None) == -1
    assert L.eg3d_host_cloud_nearest(D.np_ptr(q, C.c_float), 1, None, None, 1, None, 1.0, 0.5, None, None, None) == -1
    assert L.eg3d_host_cloud_nearest(None, 1 << 32, None, None, 0, None, 1.0, 0.5, None, None, None) == -1   # (NULL comes first)
    assert L.eg3d_host_cloud_nearest(D.np_ptr(q, C.c_float), 1 << 32, None, None, 0, None, 1.0, 0.5, None, None, None) == host.NEAREST_ERR_CAPACITY
    assert L.eg3d_host_cloud_index_stats(D.np_ptr(q, C.c_float), 1, None, 1.0, None) == -1


# ---- the PLY reader ----------------------------------------------------------------------------------------------------------------
def test_reads_back_what_write_ply_wrote(tmp_path):
    rng = np.random.default_rng(5)
    X = np.concatenate([rng.normal(0, 100, (300, 3)), rng.normal(0, 1e-3, (50, 3)), [[0, -0.0, 1e20], [1.5, -2.25, 3e-20]]]).astype(F)
    p = str(tmp_path / "cloud.ply")
    host.write_ply(p, X, rgb=rng.integers(0, 256, (len(X), 3)).astype(np.uint8))
    got = host.read_ply_points(p)
    text = open(p).read().split("end_header\n")[1].split("\n")
    want = np.array([[F(float(w)) for w in line.split()[:3]] for line in text if line], F)
    assert got.shape == X.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.allclose(got, X, rtol=1e-5, atol=0)


def _binary_ply(X, header_eol="\n", n_promised=None, fmt="binary_little_endian"):
    """uchar and float properties before, between and after x, y and z"""
    n = len(X) if n_promised is None else n_promised
    lines = ["ply", "format %s 1.0" % fmt, "comment made by a test", "element vertex %d" % n, "property uchar red", "property float x",
             "property float nx", "property uchar green", "property float y", "property double weight", "property float z", "property short tag",
             "property uchar blue", "element face 1", "property list uchar int vertex_indices", "end_header"]
    body = b"".join(struct.pack("<BffBfdfhB", i % 256, x, 0.5, 7, y, 1.25, z, -3, 9) for i, (x, y, z) in enumerate(X.tolist()))
    return (header_eol.join(lines) + header_eol).encode() + body + struct.pack("<Biii", 3, 0, 1, 2)


@pytest.mark.parametrize("eol", ["\n", "\r\n"], ids=["lf", "crlf"])
def test_reads_binary_little_endian_with_other_properties(tmp_path, eol):
    X = np.random.default_rng(6).normal(0, 10, (257, 3)).astype(F)
    p = tmp_path / "scan.ply"
    p.write_bytes(_binary_ply(X, eol))
    got = host.read_ply_points(str(p))
    assert np.array_equal(got.view(np.uint32), X.view(np.uint32))


def test_reads_ascii_with_crlf_and_other_properties_and_an_empty_vertex_element(tmp_path):
    p = tmp_path / "a.ply"
    p.write_bytes(b"ply\r\nformat ascii 1.0\r\nelement vertex 2\r\nproperty uchar red\r\nproperty float x\r\nproperty float y\r\n"
                  b"property float32 z\r\nproperty int k\r\nelement edge 1\r\nproperty int a\r\nend_header\r\n255 1.5 -2 0.1 7\r\n0 1e-3 4 5 -1\r\n3\r\n")
    assert np.array_equal(host.read_ply_points(str(p)), np.array([[1.5, -2, F(0.1)], [F(1e-3), 4, 5]], F))
    p.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    assert host.read_ply_points(str(p)).shape == (0, 3)


X2 = np.array([[1, 2, 3], [4, 5, 6]], F)
HEAD = "ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
MALFORMED = [
    ("big_endian", _binary_ply(X2, fmt="binary_big_endian"), "big-endian"),
    ("list_in_vertex", HEAD.replace("property float z\n", "property float z\nproperty list uchar int idx\n").encode() + b"1 2 3 0\n4 5 6 0\n", "list property"),
    ("no_z", HEAD.replace("property float z\n", "").encode() + b"1 2\n4 5\n", "no float property z"),
    ("double_x", HEAD.replace("float x", "double x").encode() + b"1 2 3\n4 5 6\n", "x is not a float"),
    ("no_end_header", HEAD.replace("end_header\n", "").encode() + b"1 2 3\n4 5 6\n", "does not end"),
    ("header_cut", b"ply\nformat ascii 1.0\nelement vert", "does not end"),
    ("short_ascii_body", HEAD.encode() + b"1 2 3\n4 5\n", "shorter"),
    ("short_binary_body", _binary_ply(X2, n_promised=3)[:-13], "shorter"),
    ("huge_count", HEAD.replace("vertex 2", "vertex 18446744073709551615").encode() + b"1 2 3\n", "shorter"),
    ("not_ply", b"plx\nformat ascii 1.0\n", "not a PLY"),
    ("empty_file", b"", "not a PLY"),
    ("no_number", HEAD.encode() + b"1 2 3\n4 five 6\n", "no number"),
    ("unknown_type", HEAD.replace("float y", "quad y").encode() + b"1 2 3\n4 5 6\n", "unknown property type"),
    ("no_vertex", b"ply\nformat ascii 1.0\nend_header\n", "no `element vertex`"),
]


@pytest.mark.parametrize("name,data,phrase", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_the_reader_refuses_malformed_files_with_a_message(tmp_path, name, data, phrase):
    p = tmp_path / (name + ".ply")
    p.write_bytes(data)
    X, n = D.f32p(), C.c_uint64(77)
    rc = host.lib().eg3d_host_read_ply_points(os.fsencode(str(p)), C.byref(X), C.byref(n))
    assert rc == host.NEAREST_ERR_PLY and not X and n.value == 77
    assert phrase in host.lib().eg3d_host_nearest_last_error().decode(), host.lib().eg3d_host_nearest_last_error()
    with pytest.raises(host.NearestError) as e:
        host.read_ply_points(str(p))
    assert e.value.code == host.NEAREST_ERR_PLY


def test_a_missing_file_has_its_own_code(tmp_path):
    with pytest.raises(host.NearestError) as e:
        host.read_ply_points(str(tmp_path / "nothing.ply"))
    assert e.value.code == host.NEAREST_ERR_FILE
