"""-m gpu: K15, eg3d_colour_points / eg3d_colour_device (include/eg3d_colour.h), byte for byte — colours, flags, counts and
return codes — against the host statement (eg3d_host_colour_points), once per product library:
  * every row of tests/colour_cases.py through colour_points and through colour_device on uploaded arrays (64-bit offsets
    without a sentinel), with and without the mask;
  * every refusal alone (EG3D_ERR_ARG), each followed by a valid call on the same context; refused observations on points
    the mask drops are not a refusal. No refused input forms an index: the checks run first;
  * on host.Synth(2) with seeded images of the scene's size, after match_refpoints(device_only=True): colour_device() on the
    NULL cloud, with the mask of dedup_device, and on the result of compact_device;
  * a second upload changes the colours, release_images and a clone without images are refused."""
import ctypes as C

import numpy as np
import pytest

import colour_cases as cc
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host

pytestmark = pytest.mark.gpu

V = 16
_CTX = {}    # form -> api.Context on host.Synth(5) (16 views), images of colour_cases uploaded
_KEEP = []
_HOST = {}   # table name -> the host statement's (rgb, flags, counts), computed once


@pytest.fixture(scope="module")
def have_gpu():
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"


def _ctx(form):
    if form not in _CTX:
        s = host.Synth(5)
        _KEEP.append(s)
        ctx = api.Context(s.scene)
        assert ctx.n_views == V
        ctx.upload_images(cc.images(V))
        _CTX[form] = ctx
    return _CTX[form]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    import forms
    for rows, ctx in list(_CTX.items()):
        with forms.product_form(rows):   # eg3d_destroy of the library that created the context
            ctx.close()
    _CTX.clear()
    _KEEP.clear()


def _want(name):
    if name not in _HOST:
        cloud = getattr(cc, name)(V)
        _HOST[name] = host.colour_points(cc.images(V), *cloud.args(), keep=cloud.keep, n_threads=4)
    return _HOST[name]


def _same(got, want, what):
    rgb, flags, st = got
    wrgb, wflags, wcounts = want
    bad = np.flatnonzero((rgb != wrgb).any(axis=1))
    assert not len(bad), (what, bad[:8], rgb[bad[:8]], wrgb[bad[:8]])
    assert (flags == wflags).all(), what
    assert {k: st[k] for k in wcounts} == wcounts, (what, st, wcounts)
    assert st["n_points"] == len(rgb) and st["n_images"] == V - 1, what


def _device_cloud(ctx, cloud):
    """the table as a caller-built device cloud; returns (DeviceEdgePoints, keep DeviceArray or None, what keeps them alive)"""
    m = int(cloud.obs_off[-1])
    arrays = [ctx.upload(np.zeros((cloud.n, 3), np.float32)), ctx.upload(cloud.device_offsets()),
              ctx.upload(cloud.obs_view if m else np.zeros(1, np.int32)), ctx.upload(cloud.obs_xy if m else np.zeros(2, np.float32))]
    d = D.DeviceEdgePoints(n_points=cloud.n, n_obs=m, X=arrays[0].ptr, obs_off=arrays[1].ptr, obs_view=arrays[2].ptr,
                           obs_xy=arrays[3].ptr, complete=1)
    keep = None if cloud.keep is None else ctx.upload(cloud.keep)
    return d, keep, arrays


def _colour_device(ctx, cloud):
    d, keep, alive = _device_cloud(ctx, cloud)
    rgb, flags, st = ctx.colour_device(d, keep)
    return rgb.numpy(np.uint8, (cloud.n, 3)), flags.numpy(np.uint8), st


@pytest.mark.parametrize("name", ("main", "main_masked", "dropped_bad", "valid_probe"))
def test_tables_against_the_host_statement(have_gpu, eg3d_form, name):
    ctx, cloud = _ctx(eg3d_form), getattr(cc, name)(V)
    got = ctx.colour_points(*cloud.args(), keep=cloud.keep)
    _same(got, _want(name), name + ": eg3d_colour_points")
    st = got[2]
    print("%s: %d points, %d coloured, %d empty, %d observations; sample %.3f ms, mix %.3f ms, copy %.3f ms" %
          (name, cloud.n, st["n_coloured"], st["n_empty"], st["n_obs_sampled"], st["ms_sample"], st["ms_mix"], st["ms_copy"]))
    _same(_colour_device(ctx, cloud), _want(name), name + ": eg3d_colour_device")
    if name == "main":
        assert st["n_empty"] == 1 and int(np.diff(cloud.obs_off).max()) == cc.MAX_OBS
    if cloud.keep is not None:
        assert not got[0][cloud.keep == 0].any() and not got[1][cloud.keep == 0].any()
    # without flags: the colours alone
    rgb, flags, _ = ctx.colour_device(_device_cloud(ctx, cloud)[0], None if cloud.keep is None else ctx.upload(cloud.keep),
                                      with_flags=False)
    assert flags is None and (rgb.numpy(np.uint8, (cloud.n, 3)) == _want(name)[0]).all()


def _good(ctx):
    probe = cc.valid_probe(V)
    _same(ctx.colour_points(*probe.args()), _want("valid_probe"), "the call after a refusal")


@pytest.mark.parametrize("name", sorted(cc.refusals(V)))
def test_refusals_leave_the_context_usable(have_gpu, eg3d_form, name):
    ctx, cloud = _ctx(eg3d_form), cc.refusals(V)[name]
    with pytest.raises(ValueError):
        host.colour_points(cc.images(V), *cloud.args(), keep=cloud.keep)
    with pytest.raises(api.Eg3dError) as e:
        ctx.colour_points(*cloud.args(), keep=cloud.keep)
    assert "rc=-1" in str(e.value) and "eg3d_colour_points" in str(e.value), str(e.value)
    _good(ctx)
    d, keep, alive = _device_cloud(ctx, cloud)
    with pytest.raises(api.Eg3dError) as e:
        ctx.colour_device(d, keep)
    assert "rc=-1" in str(e.value) and "eg3d_colour_device" in str(e.value), str(e.value)
    _good(ctx)


def test_refusals_of_the_call_itself(have_gpu, eg3d_form):
    ctx, probe = _ctx(eg3d_form), cc.valid_probe(V)
    L = api.lib()
    off, view, xy = probe.args()
    rgb = np.full((probe.n, 3), 7, np.uint8)
    # a stats struct that is too small: refused before anything is written
    small = D.ColourStats(struct_size=C.sizeof(D.ColourStats) - 4)
    rc = L.eg3d_colour_points(ctx._h, probe.n, D.np_ptr(off, C.c_uint32), D.np_ptr(view, C.c_int32), D.np_ptr(xy, C.c_float), None,
                              D.np_ptr(rgb, C.c_uint8), None, C.byref(small))
    assert rc == -1 and b"struct_size" in L.eg3d_last_error() and (rgb == 7).all()
    _good(ctx)
    # n_views different from the rig's at upload: refused, and the images of before stay
    with pytest.raises(api.Eg3dError) as e:
        ctx.upload_images(cc.images(V)[:-1])
    assert "rc=-1" in str(e.value) and "n_views" in str(e.value)
    _good(ctx)
    # an incomplete image list entry: a side of 0
    a = D.ImageArgs(cc.images(V))
    a.width[3] = 0
    assert L.eg3d_upload_images(ctx._h, *a.args()) == -1
    _good(ctx)


def test_images_belong_to_their_context(have_gpu, eg3d_form):
    """A second upload replaces the first; release_images and a clone without images are refused until an upload."""
    ctx, probe = _ctx(eg3d_form), cc.valid_probe(V)
    first = ctx.colour_points(*probe.args())[0]
    other = [None if im is None else (255 - im) for im in cc.images(V)]
    want_other = host.colour_points(other, *probe.args())
    assert (want_other[0] != first).any()
    clone = ctx.clone()
    try:
        with pytest.raises(api.Eg3dError) as e:
            clone.colour_points(*probe.args())
        assert "rc=-1" in str(e.value) and "no images" in str(e.value)
        with pytest.raises(api.Eg3dError):
            clone.colour_device(_device_cloud(clone, probe)[0])
        clone.upload_images(other)
        _same(clone.colour_points(*probe.args()), want_other, "the clone's own images")
        _good(ctx)                                     # ... and the parent still has its own
        ctx.upload_images(other)
        _same(ctx.colour_points(*probe.args()), want_other, "the second upload")
        ctx.release_images()
        with pytest.raises(api.Eg3dError) as e:
            ctx.colour_points(*probe.args())
        assert "rc=-1" in str(e.value) and "no images" in str(e.value)
        _same(clone.colour_points(*probe.args()), want_other, "the clone after the parent released its images")
    finally:
        clone.close()
        ctx.upload_images(cc.images(V))
    _good(ctx)


def test_resident_cloud_of_a_match(have_gpu, eg3d_form):
    s = host.Synth(2)
    sc = s.scene.contents
    Vs, W, H = int(sc.n_views), int(sc.width), int(sc.height)
    rng = np.random.default_rng(215)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(Vs)]
    ctx = api.Context(s.scene)
    try:
        ctx.upload_images(images)
        ctx.match_refpoints(s.seeds, device_only=True)
        dev = ctx.last_device_output()
        assert dev.complete == 1 and dev.n_points > 0
        cloud = ctx.fetch_device_output()
        n = int(cloud["n_points"])
        off32 = cloud["obs_off"].astype(np.uint32)
        args = (off32, cloud["obs_view"], cloud["obs_xy"])
        want = host.colour_points(images, *args, n_threads=4)
        rgb, flags, st = ctx.colour_device()
        got = rgb.numpy(np.uint8, (n, 3))
        assert (got == want[0]).all() and (flags.numpy(np.uint8) == want[1]).all()
        assert {k: st[k] for k in want[2]} == want[2] and st["n_points"] == n and st["n_images"] == Vs
        assert len(np.unique(got, axis=0)) > n // 4          # seeded bytes: the colours are not all alike
        print("Synth(2): %d points, %d observations, %dx%d images; sample %.3f ms, mix %.3f ms" %
              (n, st["n_obs_sampled"], W, H, st["ms_sample"], st["ms_mix"]))
        # the mask of the 3 px dedup
        keep, n_kept = ctx.dedup_device(dev)
        k = keep.numpy(np.uint8)
        assert 0 < n_kept == int(k.sum()) <= n
        want_k = host.colour_points(images, *args, keep=k, n_threads=4)
        rgb_k, flags_k, st_k = ctx.colour_device(None, keep)
        assert (rgb_k.numpy(np.uint8, (n, 3)) == want_k[0]).all() and (flags_k.numpy(np.uint8) == want_k[1]).all()
        assert {f: st_k[f] for f in want_k[2]} == want_k[2] and st_k["n_coloured"] + st_k["n_empty"] == n_kept
        assert (want_k[0][k != 0] == want[0][k != 0]).all() and not want_k[0][k == 0].any()
        # colouring the compacted cloud == compacting the colours
        out = ctx.compact_device(dev, keep)
        assert int(out.n_points) == n_kept
        rgb_c, _, st_c = ctx.colour_device(out)
        assert (rgb_c.numpy(np.uint8, (n_kept, 3)) == want[0][k != 0]).all()
        assert st_c["n_points"] == n_kept and st_c["n_obs_sampled"] == st_k["n_obs_sampled"]
    finally:
        ctx.close()
