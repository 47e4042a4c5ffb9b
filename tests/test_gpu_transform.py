"""-m gpu: K16, eg3d_transform_device / eg3d_transform_points (include/eg3d_transform.h), byte for byte against the host
statement (eg3d_host_transform_points), once per product library:
  * 0, 1, 63, 64, 65, 255, 256, 257 and 100 003 points — either side of the wavefront and block boundaries, the last not a
    multiple of 4 — in place and out of place, the flat arrays on a 16-byte boundary and 4, 8, 12 bytes past one (input and
    output misaligned independently); the floats in front of and behind the arrays stay as they were;
  * the mask (all, none, alternating, one bit): unkept points keep their bits;
  * on the resident cloud of host.Synth(1) after match_refpoints(device_only=True): transform -> fetch equals fetch ->
    host.transform_points, every other array untouched, the colours unchanged, T then T^-1 returns within a derived bound;
  * the counts, the library's live device bytes, and the three refusals with their own codes, the cloud unchanged after each."""
import ctypes as C

import numpy as np
import pytest

from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, host
from test_transform_host import matrices, special_points

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 100003)
GUARD = 8          # floats kept in front of and behind every test array
_REF = {}          # (matrix index, n) -> (X, the host statement's result), computed once
_CTX = {}          # form -> api.Context on host.Synth(0)
_KEEP = []


@pytest.fixture(scope="module")
def have_gpu():
    assert api.device_count() >= 1, "no HIP device: the product path has no CPU fallback"


def _ctx(form):
    if form not in _CTX:
        s = host.Synth(0)
        _KEEP.append(s)
        _CTX[form] = api.Context(s.scene)
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


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ref(k, n):
    if (k, n) not in _REF:
        base = special_points(seed=n)
        X = np.ascontiguousarray(np.tile(base, (n // len(base) + 1, 1))[:n])
        _REF[(k, n)] = (X, host.transform_points(matrices()[k], X))
    return _REF[(k, n)]


class Flat:
    """n points in a device array with GUARD marker floats on both sides, the first point `shift` floats past a 16-byte
    boundary (hipMalloc returns 256-byte aligned blocks)"""
    MARK = np.float32(-12345.5)

    def __init__(self, ctx, n, shift, X=None):
        self.n, self.first = n, GUARD + shift
        a = np.full(3 * n + 2 * GUARD + 4, self.MARK, np.float32)
        if X is not None:
            a[self.first:self.first + 3 * n] = X.reshape(-1)
        self.sent = a
        self.dev = ctx.upload(a)
        self.ptr = self.dev.ptr + 4 * self.first
        assert self.dev.ptr % 256 == 0 and (self.ptr % 16) // 4 == shift

    def read(self):
        a = self.dev.numpy(np.float32)
        body = slice(self.first, self.first + 3 * self.n)
        outside = np.ones(len(a), bool)
        outside[body] = False
        assert (_bits(a[outside]) == _bits(self.sent[outside])).all(), "a float outside the array was written"
        return a[body].reshape(self.n, 3)


def _cloud(ctx, flat):
    off = ctx.upload(np.zeros(max(flat.n, 1), np.uint64))
    return D.DeviceEdgePoints(n_points=flat.n, n_obs=0, X=flat.ptr, obs_off=off.ptr, complete=1), off


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_alignments_byte_for_byte(have_gpu, eg3d_form, n):
    ctx = _ctx(eg3d_form)
    k = 2   # the projective matrix: h[3] != 1, the division is not a no-op
    T = matrices()[k]
    X, want = _ref(k, n)
    for shift_in, shift_out in ((0, None), (1, None), (2, None), (3, None), (0, 0), (0, 3), (1, 2), (2, 0), (3, 1)):
        src = Flat(ctx, n, shift_in, X)
        dst = None if shift_out is None else Flat(ctx, n, shift_out)
        d, alive = _cloud(ctx, src)
        st = ctx.transform_device(T, out=None if dst is None else dst.ptr, cloud=d)
        got = (src if dst is None else dst).read()
        what = (n, shift_in, shift_out)
        bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
        assert not len(bad), (what, bad[:6], got[bad[:6]], want[bad[:6]])
        if dst is not None:
            assert (_bits(src.read()) == _bits(X)).all(), what   # out of place: the input stays
        assert st["n_points"] == n and st["n_transformed"] == n, (what, st)
        assert st["n_nonfinite"] == int((~np.isfinite(want)).any(axis=1).sum()), (what, st)
    # host arrays through the same kernel
    got, st = ctx.transform_points(T, X)
    assert (_bits(got) == _bits(want)).all() and st["n_transformed"] == n
    if n == 100003:
        for k2 in (0, 1):
            X2, want2 = _ref(k2, n)
            got2, _ = ctx.transform_points(matrices()[k2], X2)
            assert (_bits(got2) == _bits(want2)).all(), k2
        assert np.isnan(want).any() and n % 4 == 3


@pytest.mark.parametrize("mask", ("all", "none", "alternating", "one"))
def test_unkept_points_keep_their_bits(have_gpu, eg3d_form, mask):
    ctx, n, k = _ctx(eg3d_form), 1003, 2
    X, want = _ref(k, n)
    keep = {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "alternating": (np.arange(n) % 2).astype(np.uint8),
            "one": (np.arange(n) == 700).astype(np.uint8) * 200}[mask]
    expect = np.where(keep[:, None] != 0, _bits(want), _bits(X))
    kd = ctx.upload(keep)
    for shift_in, shift_out in ((0, None), (1, None), (0, 0), (3, 2)):
        src = Flat(ctx, n, shift_in, X)
        dst = None if shift_out is None else Flat(ctx, n, shift_out)
        d, alive = _cloud(ctx, src)
        st = ctx.transform_device(T=matrices()[k], keep=kd, out=None if dst is None else dst.ptr, cloud=d)
        got = (src if dst is None else dst).read()
        assert (_bits(got) == expect).all(), (mask, shift_in, shift_out)
        assert st["n_transformed"] == int((keep != 0).sum())
        assert st["n_nonfinite"] == int((~np.isfinite(want[keep != 0])).any(axis=1).sum())


def test_nonfinite_results_are_counted(have_gpu, eg3d_form):
    ctx, n = _ctx(eg3d_form), 5000
    X = np.float32(np.random.default_rng(4).normal(size=(n, 3)))
    for i in (0, 2047, 4999):
        X[i, i % 3] = np.nan
    T = matrices()[0]
    want = host.transform_points(T, X)
    assert int((~np.isfinite(want)).any(axis=1).sum()) == 3
    src = Flat(ctx, n, 0, X)
    d, alive = _cloud(ctx, src)
    st = ctx.transform_device(T, cloud=d)
    assert st["n_nonfinite"] == 3 and st["n_transformed"] == n and (_bits(src.read()) == _bits(want)).all()


def _live():
    f = api.lib().eg3d_test_live_device_bytes
    f.restype, f.argtypes = C.c_int64, []
    return int(f())


def test_resident_cloud_of_a_match(have_gpu, eg3d_form):
    s = host.Synth(1)
    sc = s.scene.contents
    Vs, W, H = int(sc.n_views), int(sc.width), int(sc.height)
    rng = np.random.default_rng(216)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(Vs)]
    start = _live()
    ctx = api.Context(s.scene)
    try:
        ctx.upload_images(images)
        ctx.match_refpoints(s.seeds, device_only=True)
        before = ctx.fetch_device_output()
        n = int(before["n_points"])
        assert n > 0 and _live() > start
        rgb0 = ctx.colour_device()[0].numpy(np.uint8, (n, 3))
        T = matrices()[0]   # a similarity, as host.similarity_fit returns
        want = host.transform_points(T, before["X"])
        st = ctx.transform_device(T)
        after = ctx.fetch_device_output()
        assert st["n_points"] == st["n_transformed"] == n and st["n_nonfinite"] == 0
        assert (_bits(after["X"]) == _bits(want)).all() and (_bits(want) != _bits(before["X"])).any()
        for name in before:
            if name != "X":
                assert np.array_equal(before[name], after[name]), name
        # colours depend on the observations only
        assert (ctx.colour_device()[0].numpy(np.uint8, (n, 3)) == rgb0).all()
        # the cloud still feeds the compaction
        keep, n_kept = ctx.dedup_device(ctx.last_device_output())
        out = ctx.compact_device(ctx.last_device_output(), keep)
        assert int(out.n_points) == n_kept
        # ... and T followed by the FP64 inverse of T comes back. Both matrices are affine with last row (0, 0, 0, 1), so
        # h[3] = 1 exactly and the division changes nothing. A coordinate of A x + t in FP32 carries the rounding of the
        # matrix entries (eps / 2 relative, each), of the products (eps / 2, each) and of the three additions (eps / 2 of a
        # partial sum, each): at most 2.5 eps B with B = sum_j |A_ij| |x_j| + |t_i|, eps = 2^-23 (terms in eps^2 dropped;
        # the factor 4 below covers them). The second transform multiplies the first one's error by at most
        # |A^-1|_inf and adds its own 2.5 eps B': bound = 4 eps (|A^-1|_inf B + B').
        Ti = np.linalg.inv(T)
        ctx.transform_device(Ti)
        back = ctx.fetch_device_output()["X"].astype(np.float64)
        x0 = before["X"].astype(np.float64)
        r = np.abs(x0).max()
        B = np.abs(T[:3, :3]).sum(axis=1).max() * r + np.abs(T[:3, 3]).max()
        ymax = np.abs(want.astype(np.float64)).max()
        B2 = np.abs(Ti[:3, :3]).sum(axis=1).max() * ymax + np.abs(Ti[:3, 3]).max()
        bound = 4 * 2.0 ** -23 * (np.abs(Ti[:3, :3]).sum(axis=1).max() * B + B2)
        err = np.abs(back - x0).max()
        print("Synth(1): %d points, |x| <= %.3g; T then T^-1: max error %.3g, bound %.3g; kernel %.3f ms" %
              (n, r, err, bound, st["ms_kernel"]))
        assert err <= bound
        got, _ = ctx.transform_points(T, before["X"])
        assert (_bits(got) == _bits(want)).all()
    finally:
        ctx.close()
    assert _live() == start


def test_refusals_come_before_the_launch(have_gpu, eg3d_form):
    ctx, n = _ctx(eg3d_form), 300
    X, _ = _ref(0, n)
    T = matrices()[0]
    src = Flat(ctx, n, 0, X)
    d, alive = _cloud(ctx, src)
    room = Flat(ctx, 2 * n, 0)

    def untouched():
        assert (_bits(src.read()) == _bits(X)).all()
        room.read()

    bad = T.copy()
    bad[2, 1] = np.nan
    with pytest.raises(api.Eg3dError) as e:
        ctx.transform_device(bad, cloud=d)
    assert "rc=%d" % api.ERR_TRANSFORM_NONFINITE in str(e.value) and "T[9]" in str(e.value), str(e.value)
    untouched()
    big = T.copy()
    big[0, 3] = 1e300   # finite as a double, an infinity as a float
    with pytest.raises(api.Eg3dError) as e:
        ctx.transform_points(big, X)
    assert "rc=%d" % api.ERR_TRANSFORM_NONFINITE in str(e.value)
    with pytest.raises(ValueError):
        ctx.transform_device(T, keep=ctx.upload(np.ones(n - 1, np.uint8)), cloud=d)
    untouched()
    with pytest.raises(ValueError):
        ctx.transform_device(T, out=api.DeviceArray(12 * n + 4), cloud=d)
    untouched()
    for delta in (4, 12 * n - 4, -8):   # X_out inside, at the end of, and in front of X: each overlaps it in part
        with pytest.raises(api.Eg3dError) as e:
            ctx.transform_device(T, out=src.ptr + delta, cloud=d)
        assert "rc=%d" % api.ERR_TRANSFORM_OVERLAP in str(e.value) and "overlaps" in str(e.value), str(e.value)
        untouched()
    assert len({api.ERR_TRANSFORM_NONFINITE, api.ERR_TRANSFORM_OVERLAP, -1}) == 3
    small = D.TransformStats(struct_size=C.sizeof(D.TransformStats) - 4)
    Tc = np.ascontiguousarray(T, np.float64)
    rc = api.lib().eg3d_transform_device(ctx._h, C.byref(d), D.np_ptr(Tc, C.c_double), None, None, C.byref(small))
    assert rc == -1 and b"struct_size" in api.lib().eg3d_last_error()
    untouched()
    # the context serves a valid call after the refusals
    st = ctx.transform_device(T, out=room.ptr, cloud=d)
    assert st["n_transformed"] == n and (_bits(room.read()[:n]) == _bits(host.transform_points(T, X))).all()
