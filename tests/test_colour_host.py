"""No GPU: the host statement of include/eg3d_host_colour.h against the independent restatement of tests/colour_ref.py.
  * eg3d_host_colour_points on every row of tests/colour_cases.py: colours, flags, counts and refusals;
  * the closed form of the border rule the kernel uses (the host compilation of csrc/eg3d_dev_colour.h) against the loop,
    in C and in Python, for every p in [-4 len - 3, 4 len + 3], len 1 .. 9;
  * eg3d_host_write_ply byte for byte; eg3d_host_png_read_rgb on PNG files written here with zlib;
  * what the two colour headers promise beyond their signatures (those are held by tests/test_abi.py): the flag, the stated
    deviations, the named fields, the build guard's bound on K15."""
import json
import os
import re
import struct
import zlib

import numpy as np
import pytest

import colour_cases as cc
import colour_ref as cr
import test_abi
from edgegraph3d_amd import api, build, host

V = 16
_REF = {}


def reference(name, cloud):
    """colour_ref.colour on a shared table, computed once"""
    if name not in _REF:
        _REF[name] = cr.colour(cc.images(V), *cloud.args(), keep=cloud.keep)
    return _REF[name]


@pytest.mark.parametrize("threads", (1, 4))
@pytest.mark.parametrize("name", ("main", "main_masked", "dropped_bad", "valid_probe"))
def test_host_statement_equals_the_restatement(name, threads):
    cloud = getattr(cc, name)(V)
    refused, rgb, flags, counts = reference(name, cloud)
    assert not refused
    got_rgb, got_flags, got_counts = host.colour_points(cc.images(V), *cloud.args(), keep=cloud.keep, n_threads=threads)
    bad = np.flatnonzero((got_rgb != rgb).any(axis=1))
    assert not len(bad), (name, bad[:8], got_rgb[bad[:8]], rgb[bad[:8]])
    assert (got_flags == flags).all() and got_counts == counts
    if cloud.keep is not None:
        dropped = cloud.keep == 0
        assert dropped.any() and not got_rgb[dropped].any() and not got_flags[dropped].any()
    if name == "main":
        assert counts["n_empty"] == 1 and flags.sum() == cr.FLAG_EMPTY
        assert int(np.diff(cloud.obs_off).max()) == cr.MAX_OBS
        print("main: %d points, %d observations, %d distinct colours" % (cloud.n, counts["n_obs_sampled"], len(np.unique(rgb, axis=0))))


def test_the_rows_do_what_they_are_there_for():
    """ties to even, the low byte of an out-of-range rounded sum, the integer mean"""
    cloud, (refused, rgb, _, _) = cc.main(V), reference("main", cc.main(V))
    ims = cc.images(V)
    t = cc.ties_view(V)
    assert cr.sample(ims[t], 0.5, 0.0) == [0, 0, 0] and cr.sample(ims[t], 1.5, 0.0) == [2, 2, 2]
    assert cr.sample(ims[t], 3.5, 0.0) == [254, 254, 254]
    # 3x2 checkerboard, px = -0.5: x = 0, a = -0.5 -> 255 * 1.5 = 382.5 -> 382 -> 126, and 255 * -0.5 = -127.5 -> -128 -> 128
    assert sorted(set(cr.sample(ims[4], -0.5, 0.0))) == [126, 128]
    two = [i for i in range(cloud.n) if list(cloud.obs_xy[cloud.obs_off[i]:cloud.obs_off[i + 1]].ravel()) == [4.0, 0.0, 3.0, 0.0]]
    assert len(two) == 1 and list(rgb[two[0]]) == [254, 254, 254]


@pytest.mark.parametrize("name", sorted(cc.refusals(V)))
def test_refusals(name):
    cloud = cc.refusals(V)[name]
    assert cr.colour(cc.images(V), *cloud.args(), keep=cloud.keep)[0]
    with pytest.raises(ValueError):
        host.colour_points(cc.images(V), *cloud.args(), keep=cloud.keep, n_threads=2)


def test_closed_form_of_the_border_rule_equals_the_loop():
    L = host.lib()
    n = 0
    for length in range(1, 10):
        for p in range(-4 * length - 3, 4 * length + 4):
            want = cr.reflect101(p, length)
            assert 0 <= want < length
            assert L.eg3d_host_reflect101_loop(p, length) == want, (p, length)
            assert L.eg3d_host_reflect101_closed(p, length) == want, (p, length)
            n += 1
    assert n == sum(8 * l + 7 for l in range(1, 10))
    for p, length in ((9999999, 7), (-9999999, 5), (10000000, 2), (-10000000, 32768), (12345, 1)):
        assert L.eg3d_host_reflect101_closed(p, length) == L.eg3d_host_reflect101_loop(p, length), (p, length)


# ---- the PLY writer ------------------------------------------------------------------------------------------------------
def _written(tmp_path, X, rgb=None, keep=None):
    path = tmp_path / "cloud.ply"
    host.write_ply(str(path), X, rgb, keep)
    return path.read_bytes()


def test_write_ply_formats_floats_as_the_stream_does(tmp_path):
    X, rgb = cc.ply_points()
    for text, value in (("0", 0.0), ("-0", -0.0), ("1e-05", 1e-5), ("123457", 123456.7), ("1.23457e+06", 1234567.0),
                        ("1.4013e-45", 1e-45), ("nan", float("nan")), ("inf", float("inf")), ("-inf", float("-inf"))):
        assert cr.g_text(value) == text
    got = _written(tmp_path, X, rgb)
    assert got == cr.ply_bytes(X, rgb)
    assert got.count(b"\n") == 10 + len(X) - 1 and not got.endswith(b"\n")
    assert b"element vertex %d\n" % len(X) in got
    assert _written(tmp_path, X) == cr.ply_bytes(X)             # uncoloured: 255 255 255
    assert _written(tmp_path, X).endswith(b" 255 255 255")


def test_write_ply_sizes_zero_and_one(tmp_path):
    head = cr.ply_bytes(np.zeros((0, 3), np.float32))
    assert _written(tmp_path, np.zeros((0, 3), np.float32)) == head and head.endswith(b"end_header\n") and head.count(b"\n") == 10
    one = _written(tmp_path, np.array([[1.5, -2.0, 1e-5]], np.float32), np.array([[1, 2, 3]], np.uint8))
    assert one == cr.ply_bytes([[1.5, -2.0, 1e-5]], [[1, 2, 3]]) and one.endswith(b"end_header\n1.5 -2 1e-05 1 2 3")


@pytest.mark.parametrize("last_kept", (True, False))
def test_write_ply_inliers_form(tmp_path, last_kept):
    X, rgb = cc.ply_points()
    keep = np.ones(len(X), np.uint8)
    keep[[0, 4, 5]] = 0
    keep[-1] = 1 if last_kept else 0
    for colours in (rgb, None):
        got = _written(tmp_path, X, colours, keep)
        assert got == cr.ply_bytes(X, colours, keep)
        assert b"element vertex %d\n" % int(keep.sum()) in got
        assert got.endswith(b"\n") == (not last_kept)   # the test is on the INDEX of the point, not on the last line written
        assert got.count(b"\n") == 10 + int(keep.sum()) - (1 if last_kept else 0)


# ---- the PNG reader ------------------------------------------------------------------------------------------------------
def _png(path, w, h, depth, ctype, rows, plte=None):
    """rows: the unfiltered scanline bytes; filter 0 on even rows, `up` on odd ones (so both run)"""
    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xffffffff)
    raw = b""
    for r, line in enumerate(rows):
        if r % 2 == 0:
            raw += b"\x00" + bytes(line)
        else:
            raw += b"\x02" + bytes((int(a) - int(b)) & 0xff for a, b in zip(line, rows[r - 1]))
    data = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0))
    if plte is not None:
        data += chunk(b"PLTE", bytes(plte))
    z = zlib.compress(raw)
    data += chunk(b"IDAT", z[:5]) + chunk(b"IDAT", z[5:]) + chunk(b"IEND", b"")
    path.write_bytes(data)
    return str(path)


def test_png_read_rgb(tmp_path):
    rng = np.random.default_rng(7)
    W, H = 3, 2
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    # RGB8
    got = host.read_png_rgb(_png(tmp_path / "rgb8.png", W, H, 8, 2, [rgb[r].ravel() for r in range(H)]))
    assert got.shape == (H, W, 3) and (got == rgb).all()
    # RGBA8: alpha dropped
    rgba = np.concatenate([rgb, rng.integers(0, 256, (H, W, 1), dtype=np.uint8)], axis=2)
    assert (host.read_png_rgb(_png(tmp_path / "rgba8.png", W, H, 8, 6, [rgba[r].ravel() for r in range(H)])) == rgb).all()
    # grey 8: replicated
    grey = rng.integers(0, 256, (H, W), dtype=np.uint8)
    got = host.read_png_rgb(_png(tmp_path / "g8.png", W, H, 8, 0, [grey[r] for r in range(H)]))
    assert (got == grey[:, :, None]).all()
    # grey 1: bits 1 0 1 / 0 1 1, scaled to 0 / 255
    got = host.read_png_rgb(_png(tmp_path / "g1.png", W, H, 1, 0, [[0b10100000], [0b01100000]]))
    assert (got[:, :, 0] == np.array([[255, 0, 255], [0, 255, 255]])).all() and (got == got[:, :, :1]).all()
    # palette, 8-bit indices
    plte = rng.integers(0, 256, (4, 3), dtype=np.uint8)
    idx = np.array([[0, 3, 1], [2, 2, 0]], np.uint8)
    got = host.read_png_rgb(_png(tmp_path / "p8.png", W, H, 8, 3, [idx[r] for r in range(H)], plte.ravel()))
    assert (got == plte[idx]).all()
    # RGB16: the high byte
    lo = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rows16 = [np.stack([rgb[r].ravel(), lo[r].ravel()], axis=1).ravel() for r in range(H)]
    assert (host.read_png_rgb(_png(tmp_path / "rgb16.png", W, H, 16, 2, rows16)) == rgb).all()
    with pytest.raises(ValueError):
        host.read_png_rgb(str(tmp_path / "missing.png"))


# ---- what the two headers promise beyond their signatures ------------------------------------------------------------------------
HEADER, HOST_HEADER = "eg3d_colour.h", "eg3d_host_colour.h"


def test_the_header_states_the_flag_and_the_deviations():
    text = open(os.path.join(test_abi.INC, HEADER)).read()   # (header_text drops the preprocessor lines)
    assert re.search(r"#define\s+EG3D_COLOUR_FLAG_EMPTY\s+1u\b", text)
    assert api.COLOUR_FLAG_EMPTY == 1
    for phrase in ("A clone (eg3d_clone) does NOT inherit them", "n == 0 is undefined behaviour in the reference", "JPEG is not read",
                   "the integer division"):
        assert phrase in text, phrase
    assert "JPEG is not read" in open(os.path.join(test_abi.INC, HOST_HEADER)).read()


def test_the_stats_keep_their_named_fields_and_the_wrappers_are_there():
    fields = test_abi.header_structs((HEADER,))["eg3d_colour_stats"]
    for f in ("n_points", "n_coloured", "n_empty", "n_obs_sampled", "ms_sample", "ms_mix", "ms_copy"):
        assert f in fields, f
    for f in ("colour_points", "write_ply", "read_png_rgb"):
        assert callable(getattr(host, f)), f
    for m in ("upload_images", "release_images", "colour_device", "colour_points"):
        assert callable(getattr(api.Context, m)), m


def test_the_build_guard_holds_k15():
    """No spilled register, no scratch and no LDS in either K15 kernel; the VGPR bounds are the build's counts."""
    b = build.RESOURCE_BOUNDS["k15_"]
    assert b["vgpr_spill_count"] == 0 and b["sgpr_spill_count"] == 0
    assert b["private_segment_fixed_size"] == 0 and b["group_segment_fixed_size"] == 0
    for k in ("k15_sample", "k15_mix"):
        assert 0 < build.RESOURCE_BOUNDS[k]["vgpr_count"] <= 64, k
    for lib in ("libeg3d", "libeg3d_dlt4x4"):
        rec = json.load(open(os.path.join(build.ROOT, "profiles", "kernel_resources_%s.json" % lib)))
        k15 = {n: r for n, r in rec.items() if "k15_" in n}
        assert len(k15) == 2, sorted(k15)
        for n, r in k15.items():
            key = "k15_sample" if "k15_sample" in n else "k15_mix"
            assert r["vgpr_count"] <= build.RESOURCE_BOUNDS[key]["vgpr_count"], n
            assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, n
