"""include/eg3d_host_transform.h against tests/transform_ref.py (an independent numpy restatement). No GPU.

The fit is FP64 and unpinned: the library's one-sided Jacobi and numpy.linalg.svd differ by rounding only. Measured on the
CPU over seeds 0 .. 999 of _similarity() for each of 3, 4, 25 and 200 centres, as max |T_host - T_numpy| / max(1, max |T|):
    n = 3: 3.95e-14    n = 4: 3.10e-14    n = 25: 5.79e-15    n = 200: 4.97e-15
(the gap to the similarity the centres were made with is 1.65e-14 at worst). FIT_TOL is ten times the worst gap: it is
there to catch a wrong formula, not a last-bit difference. Everything after the conversion of T to FP32 is bit for bit."""
import numpy as np
import pytest

import transform_ref as tr
from edgegraph3d_amd import host

FIT_TOL = 4e-13


def _similarity(seed, n):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.1, 10)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 2] = -Q[:, 2]
    t = rng.normal(size=3) * 10
    src = rng.normal(size=(n, 3)) * 5
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = c * Q, t
    return src, c * src @ Q.T + t, T


def _gap(A, B):
    return np.abs(A - B).max() / max(1.0, np.abs(B).max())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n", (3, 4, 25, 200))
def test_fit_recovers_a_known_similarity(n):
    worst = 0.0
    for seed in range(50):
        src, dst, T_true = _similarity(seed, n)
        T, st = host.similarity_fit(src, dst)
        T_np, c_np, d_np, refl = tr.umeyama(src, dst)
        worst = max(worst, _gap(T, T_np))
        assert _gap(T, T_np) <= FIT_TOL and _gap(T, T_true) <= FIT_TOL, (seed, _gap(T, T_np), _gap(T, T_true))
        assert st["n_used"] == n and not st["reflection"] and not st["rank_deficient"]
        assert n == 3 or not refl   # (three centres span a plane: the sign numpy's SVD gives the null direction is arbitrary)
        assert abs(st["scale"] - c_np) <= FIT_TOL * max(1.0, c_np)
        assert np.abs(st["singular"] - d_np).max() <= FIT_TOL * max(1.0, d_np[0])
        assert (np.diff(st["singular"]) <= 0).all()
        assert (T[3] == [0, 0, 0, 1]).all()
    print("n = %d: worst gap to numpy %.3g (bound %.3g)" % (n, worst, FIT_TOL))


def test_reflection_branch_still_gives_a_rotation():
    src, dst, _ = _similarity(7, 25)
    mirrored = dst * [1, 1, -1]
    T, st = host.similarity_fit(src, mirrored)
    T_np, c_np, _, refl = tr.umeyama(src, mirrored)
    assert st["reflection"] and refl
    R = T[:3, :3] / st["scale"]
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    assert _gap(T, T_np) <= FIT_TOL
    T2, st2 = host.similarity_fit(src, dst)
    assert not st2["reflection"] and st["scale"] < st2["scale"]   # the best ROTATION onto a mirror image shrinks


def test_null_cameras_take_no_part_and_are_left_alone(tmp_path):
    rng = np.random.default_rng(3)
    n = 9
    src, dst, T_true = _similarity(11, n)
    R = np.tile(np.eye(3, dtype=np.float32).reshape(9), (n, 1))
    C = src.astype(np.float32)
    for v in (2, 6):
        R[v], C[v] = 0, 0
    only_centre = 4   # centre 0 but a rotation: NOT a null camera
    C[only_centre] = 0
    mask = host.null_cameras(R, C)
    assert mask.tolist() == [0, 0, 1, 0, 0, 0, 1, 0, 0]
    assert [tr.is_null(R[v], C[v]) for v in range(n)] == [bool(m) for m in mask]
    # the file's triples of the null cameras are consumed: a marker there must not move the fit
    target = dst.copy()
    target[mask == 1] = 1e9
    p = tmp_path / "poses.txt"
    p.write_text("\n".join("%r\t%r   %r" % tuple(float(x) for x in row) for row in target) + "\n")
    read = host.read_camera_poses(str(p), n)
    assert (read == target).all()
    src64 = C.astype(np.float64)
    T, st = host.similarity_fit(src64, read, mask)
    T_np = tr.umeyama(src64, read, mask)[0]
    assert st["n_used"] == n - 2 and _gap(T, T_np) <= FIT_TOL
    t = rng.normal(size=(n, 3)).astype(np.float32)
    t[mask == 1] = 0
    fpp = np.tile(np.float32([800, 320, 240]), (n, 1))
    R2, C2, t2, P2 = host.transform_cameras(T, fpp, R, C, t)
    for v in np.flatnonzero(mask):
        assert not R2[v].any() and not C2[v].any() and not t2[v].any() and not P2[v].any()
    assert (R2[mask == 0] != R[mask == 0]).any()
    # the error: null cameras add nothing to the sum but count in the division (Q16)
    e = host.camera_errors(C, read, mask)
    d = np.linalg.norm(C[mask == 0].astype(np.float64) - read[mask == 0], axis=1)
    assert abs(float(e) - d.sum() / n) <= 1e-6 * d.sum() / n
    assert abs(float(e) - d.mean()) > 0.1 * d.mean()


def test_collinear_centres_do_not_crash():
    s = np.linspace(-3, 3, 12)
    src = np.outer(s, [1.0, 2.0, -0.5]) + [4, 5, 6]
    dst = np.outer(2.5 * s, [0.0, 1.0, 1.0]) / np.sqrt(2) * np.linalg.norm([1, 2, -0.5]) + [1, 1, 1]
    T, st = host.similarity_fit(src, dst)
    assert st["rank_deficient"] and st["singular"][1] <= 1e-12 * st["singular"][0]
    assert np.isfinite(T).all() and abs(st["scale"] - 2.5) < 1e-12
    R = T[:3, :3] / st["scale"]
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    moved = src @ T[:3, :3].T + T[:3, 3]
    assert np.abs(moved - dst).max() < 1e-12 * 20   # the line itself is mapped exactly; the roll about it is free
    # a planar set (rank 2) is NOT deficient: its answer is unique
    src, dst, T_true = _similarity(5, 3)
    assert not host.similarity_fit(src, dst)[1]["rank_deficient"]


def test_each_refusal_has_its_own_code(tmp_path):
    src, dst, _ = _similarity(1, 5)
    with pytest.raises(host.TransformError) as e:
        host.similarity_fit(src[:2], dst[:2])
    assert e.value.rc == host.TRANSFORM_ERR_FEW == -2
    with pytest.raises(host.TransformError) as e:
        host.similarity_fit(src, dst, [0, 1, 1, 0, 1])          # 2 non-null cameras
    assert e.value.rc == host.TRANSFORM_ERR_FEW
    with pytest.raises(host.TransformError) as e:
        host.similarity_fit(np.tile(src[0], (5, 1)), dst)
    assert e.value.rc == host.TRANSFORM_ERR_DEGENERATE == -3
    bad = src.copy()
    bad[3, 1] = np.nan
    with pytest.raises(host.TransformError) as e:
        host.similarity_fit(bad, dst)
    assert e.value.rc == host.TRANSFORM_ERR_NONFINITE == -4
    with pytest.raises(host.TransformError) as e:
        host.similarity_fit(src, np.where(bad != bad, np.inf, dst))
    assert e.value.rc == host.TRANSFORM_ERR_NONFINITE
    assert host.similarity_fit(bad, dst, [0, 0, 0, 1, 0])[1]["n_used"] == 4   # a NaN in a null camera's row is not read
    p = tmp_path / "short.txt"
    p.write_text("1 2 3\n4 5 6\n7 8\n")
    assert host.read_camera_poses(str(p), 2).tolist() == [[1, 2, 3], [4, 5, 6]]
    with pytest.raises(host.TransformError) as e:
        host.read_camera_poses(str(p), 3)
    assert e.value.rc == host.TRANSFORM_ERR_SHORT == -6
    with pytest.raises(host.TransformError) as e:
        host.read_camera_poses(str(tmp_path / "missing.txt"), 3)
    assert e.value.rc == host.TRANSFORM_ERR_FILE == -5
    assert len({host.TRANSFORM_ERR_ARG, host.TRANSFORM_ERR_FEW, host.TRANSFORM_ERR_DEGENERATE, host.TRANSFORM_ERR_NONFINITE,
                host.TRANSFORM_ERR_FILE, host.TRANSFORM_ERR_SHORT}) == 6
    Tnan = np.eye(4)
    Tnan[1, 2] = np.nan
    with pytest.raises(host.TransformError) as e:
        host.transform_cameras(Tnan, np.ones((1, 3)), np.eye(3).reshape(1, 9), np.ones((1, 3)), np.ones((1, 3)))
    assert e.value.rc == host.TRANSFORM_ERR_NONFINITE


def special_points(seed=0, n=4000):
    """random points, then the values a float can go wrong on: zeros of both signs, denormals, the largest and smallest
    normals, infinities and NaNs with payloads, each in each coordinate"""
    rng = np.random.default_rng(seed)
    X = (rng.normal(size=(n, 3)) * rng.choice([1e-3, 1, 50, 1e6], size=(n, 1))).astype(np.float32)
    bits = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x00800000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000,
                     0x7fc00000, 0xffc00001, 0x7fc12345, 0x3f800000, 0x5f000000, 0xdf000000], np.uint32).view(np.float32)
    rows = []
    for k in range(3):
        for b in bits:
            r = np.float32([1.5, -2.25, 3.0])
            r[k] = b
            rows.append(r)
    rows.append(np.float32([bits[2]] * 3))
    rows.append(np.float32([bits[5]] * 3))
    return np.concatenate([np.array(rows, np.float32), X])


def matrices():
    """a fitted similarity, one with small and large entries, and a projective last row (h[3] != 1: the division matters)"""
    out = [_similarity(2, 25)[2]]
    A = np.eye(4)
    A[:3, :3] = [[1e-20, 3e10, -7], [0.5, 1e-30, 2e5], [-1, 1, 1e-3]]
    A[:3, 3] = [1e15, -1e-15, 0]
    out.append(A)
    B = _similarity(4, 25)[2].copy()
    B[3] = [0.01, -0.02, 0.005, 0.75]
    out.append(B)
    return out


@pytest.mark.parametrize("k", range(3))
def test_transform_points_bit_for_bit(k):
    T, X = matrices()[k], special_points()
    want = tr.transform_points(T, X)
    got = host.transform_points(T, X)
    bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
    assert not len(bad), (bad[:5], X[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert np.isnan(got).any() and np.isinf(got).any() and np.isfinite(got).all(axis=1).sum() > 3000
    one = np.array([tr._point(np.asarray(T).astype(np.float32), x) for x in X[:60]], np.float32)   # the scalar statement
    assert (_bits(one) == _bits(got[:60])).all()
    inplace = X.copy()
    assert host.transform_points(T, inplace, out=inplace) is inplace and (_bits(inplace) == _bits(want)).all()
    big = np.tile(X, (40, 1))                                   # above the size at which the host statement threads
    assert len(big) > (1 << 16) and (_bits(host.transform_points(T, big)) == _bits(np.tile(want, (40, 1)))).all()


def _rig(seed, n):
    rng = np.random.default_rng(seed)
    R = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(n)]).astype(np.float32).reshape(n, 9)
    C = (rng.normal(size=(n, 3)) * 4).astype(np.float32)
    t = np.stack([-(R[v].reshape(3, 3) @ C[v]) for v in range(n)]).astype(np.float32)
    fpp = np.stack([rng.uniform(500, 3000, n), rng.uniform(200, 900, n), rng.uniform(200, 700, n)], axis=1).astype(np.float32)
    return fpp, R, C, t


@pytest.mark.parametrize("k", range(3))
def test_transform_cameras_bit_for_bit(k):
    T = matrices()[k]
    fpp, R, C, t = _rig(k, 40)
    R[5], C[5], t[5] = 0, 0, 0
    want = tr.transform_cameras(T, fpp, R, C, t)
    got = host.transform_cameras(T, fpp, R, C, t)
    for name, g, w in zip(("R", "C", "t", "P"), got, want):
        assert (_bits(g) == _bits(w)).all(), (name, np.argwhere(_bits(g) != _bits(w))[:4])
    M = np.asarray(T).astype(np.float32)
    assert (_bits(host.glm_inverse4(M)) == _bits(tr.glm_inverse(M))).all()
    A, B = np.float32(np.random.default_rng(k).normal(size=(2, 4, 4)))
    assert (_bits(host.glm_mul4(A, B)) == _bits(tr.glm_mul(A, B))).all()
    if k == 0:   # a similarity: the new camera still projects the moved points where the old one projected the old ones
        X = np.float32(np.random.default_rng(9).normal(size=(20, 3)))
        Xn = host.transform_points(T, X)
        for v in (0, 7):
            P0 = host_camera_matrix(fpp[v], R[v], t[v])
            a, b = _project(P0, X), _project(got[3][v].reshape(4, 4), Xn)
            assert np.abs(a - b).max() < 0.05, (v, np.abs(a - b).max())
    assert (got[1][5] == 0).all() and (got[3][5] == 0).all()


def host_camera_matrix(fpp, R, t):
    K = np.array([[fpp[0], 0, fpp[1]], [0, fpp[0], fpp[2]], [0, 0, 1]], np.float64)
    E = np.concatenate([R.reshape(3, 3).astype(np.float64), t.reshape(3, 1).astype(np.float64)], axis=1)
    return np.concatenate([K @ E, np.zeros((1, 4))])


def _project(P, X):
    h = np.concatenate([X.astype(np.float64), np.ones((len(X), 1))], axis=1) @ np.asarray(P, np.float64).reshape(4, 4).T
    return h[:, :2] / h[:, 2:3]


def test_camera_errors_keep_the_quirk_and_the_float_accumulator():
    rng = np.random.default_rng(21)
    n = 300
    C = (rng.normal(size=(n, 3)) * 100).astype(np.float32)
    target = C.astype(np.float64) + rng.normal(size=(n, 3)) * 1e-3 + 1000.0
    mask = (rng.random(n) < 0.3).astype(np.uint8)
    for m in (None, mask):
        got, want = host.camera_errors(C, target, m), tr.camera_errors(C, target, m)
        assert got.dtype == np.float32 and _bits(got) == _bits(want), (got, want)
    # the accumulator is a float: the FP64 sum of the same norms rounds elsewhere
    d = np.linalg.norm(C.astype(np.float64) - target, axis=1)
    assert float(host.camera_errors(C, target)) != float(np.float32(d.sum() / n))
    # Q16: the divisor is ALL cameras
    assert abs(float(host.camera_errors(C, target, mask)) * n / d[mask == 0].sum() - 1) < 1e-5
