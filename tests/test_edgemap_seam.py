"""-m gpu: edge_matching() with detect_edges (include/eg3d_edge_matcher.hpp) through examples/edge_matching_main.cpp
--detect-edges, on a toy rendered scene in the style of tests/real_scene.py cfg 1: the polylines of synthetic config 1
drawn into RGB photographs, which the test writes as PNG. The run never opens the edge folder, writes edge maps equal to
host.edge_maps of the same photographs, and a cloud. The other branch of the option — no flag, the edge folder holding
those maps — gives byte-identical JSON files: what the program did before the option existed, on the same inputs."""
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import cbuild
import png_util
import real_scene as rs
from edgegraph3d_amd import host

pytestmark = pytest.mark.gpu
LOW, HIGH, PASSES = 40, 100, 1


def write_png_rgb(path, rgb):
    """[H, W, 3] uint8 -> an 8-bit RGB PNG, no filtering."""
    h, w, _ = rgb.shape
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) +
                chunk(b"IEND", b""))


def photograph(mask, seed):
    """dark 1 pixel lines where the mask is set, on a shaded background, each channel with its own gain, under seeded noise"""
    h, w = mask.shape
    yy, xx = np.mgrid[0:h, 0:w]
    g = 150.0 + 30.0 * xx / w + 20.0 * yy / h - 110.0 * mask
    rgb = np.stack([g, 0.9 * g + 10, 0.8 * g + 30], -1) + np.random.default_rng(seed).integers(-3, 4, (h, w, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8)


def _n_points(path):
    return len(json.load(open(path))["structure"])


def test_edge_matching_main_detects_its_edge_maps(tmp_path):
    maker = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path, lib=cbuild.DEFAULT_LIB)
    exe = cbuild.build_caller("examples/edge_matching_main.cpp", tmp_path)       # (the product library of the form under test)
    d = str(tmp_path)
    env = dict(os.environ, EG3D_LIB="")
    subprocess.check_call([maker, "--make-synthetic", "1", d], env=env)
    s = host.Synth(1)
    sc = s.scene_np()
    names = [os.path.basename(v["filename"] if "filename" in v else v["value"]["ptr_wrapper"]["data"]["filename"])
             for v in json.load(open(os.path.join(d, "input.json")))["views"]]
    assert len(names) == sc["n_views"]
    images, out_a, out_b = (os.path.join(d, n) for n in ("images", "out_a", "out_b"))
    for folder in (images, out_a, out_b):
        os.makedirs(folder)
    photos = []
    for v in range(sc["n_views"]):
        a, b = int(sc["view_pl_off"][v]), int(sc["view_pl_off"][v + 1])
        off = sc["pl_vtx_off"][a:b + 1].astype(np.int64)
        photos.append(photograph(rs.rasterise(sc["vtx_xy"], off, sc["pl_valid"][a:b], sc["width"], sc["height"]), v))
        write_png_rgb(os.path.join(images, names[v]), photos[v])
    want, stats = host.edge_maps(photos, LOW, HIGH, PASSES)
    assert stats["n_edges"] > 100 * sc["n_views"]

    # the option set: the edge folder does not even exist
    run = subprocess.run([exe, images, os.path.join(d, "no_such_folder"), os.path.join(d, "input.json"), out_a + os.sep,
                          os.path.join(d, "a.json"), "--detect-edges", str(LOW), str(HIGH), "--edge-smooth", str(PASSES)],
                         env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "edge maps: detected on the device" in run.stdout and "edge_matching returned 0" in run.stdout
    for v in range(sc["n_views"]):
        path = os.path.join(out_a, names[v])
        assert np.array_equal(host.png_edge_mask(path), want[v]), names[v]
        assert np.array_equal(np.asarray(png_util.read_png_edge_mask(path)), want[v]), names[v]
    n_in = _n_points(os.path.join(d, "input.json"))
    assert _n_points(os.path.join(d, "a.json")) > n_in                 # a cloud: edge-points were added to the seeds

    # the option clear: the maps just written are the edge folder, and the program does what it always did with one
    run = subprocess.run([exe, images, out_a, os.path.join(d, "input.json"), out_b + os.sep, os.path.join(d, "b.json")],
                         env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "edge maps" not in run.stdout
    assert sorted(os.listdir(out_b)) == ["before_filtering.json"]      # no maps are written without the option
    assert open(os.path.join(d, "a.json"), "rb").read() == open(os.path.join(d, "b.json"), "rb").read()
    assert open(os.path.join(out_a, "before_filtering.json"), "rb").read() == open(os.path.join(out_b, "before_filtering.json"), "rb").read()
    # ... and without the option a missing edge folder is the failure it always was
    run = subprocess.run([exe, images, os.path.join(d, "no_such_folder"), os.path.join(d, "input.json"), out_b + os.sep,
                          os.path.join(d, "c.json")], env=env, capture_output=True, text=True)
    assert run.returncode == 1 and "edge_matching returned -1" in run.stdout
    s.close()
