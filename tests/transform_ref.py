"""An independent numpy restatement of include/eg3d_host_transform.h, for the tests: the fit through numpy.linalg.svd in
FP64 (a different SVD from the library's Jacobi, on purpose), the point and camera arithmetic in np.float32 with every sum
written out term by term in the order the header states. Nothing here calls the library."""
import numpy as np

F = np.float32


def umeyama(src, dst, null_mask=None):
    """(T [4, 4] float64, scale, singular values, reflection) of the similarity that maps src onto dst (Umeyama 1991)."""
    src, dst = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(dst, np.float64).reshape(-1, 3)
    if null_mask is not None:
        use = np.asarray(null_mask).reshape(-1) == 0
        src, dst = src[use], dst[use]
    n = len(src)
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    a, b = src - ms, dst - md
    var = (a * a).sum() / n
    sigma = b.T @ a / n
    U, d, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    reflection = np.linalg.det(U) * np.linalg.det(Vt) < 0
    if reflection:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    c = (d * S).sum() / var
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = md - c * (R @ ms)
    return T, c, d, bool(reflection)


def _point(M, p):
    """vec4(p, 1) * M and the division, FP32, left to right; M [4, 4] float32, p three float32"""
    x, y, z, w = F(p[0]), F(p[1]), F(p[2]), F(1.0)
    h = [F(F(F(F(M[j, 0] * x) + F(M[j, 1] * y)) + F(M[j, 2] * z)) + F(M[j, 3] * w)) for j in range(4)]
    return [F(h[0] / h[3]), F(h[1] / h[3]), F(h[2] / h[3])]


def transform_points(T, X):
    """X [n, 3] float32 through T; vectorised over the points, the same operations in the same order as _point"""
    M = np.asarray(T, np.float64).reshape(4, 4).astype(F)
    X = np.asarray(X, F).reshape(-1, 3)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(all="ignore"):
        h = [((M[j, 0] * x + M[j, 1] * y) + M[j, 2] * z) + M[j, 3] * F(1.0) for j in range(4)]
        out = np.stack([h[0] / h[3], h[1] / h[3], h[2] / h[3]], axis=1)
    assert out.dtype == F
    return out


def glm_inverse(m):
    """glm::inverse(mat4) of glm 0.9.6 (the cofactor form), m[i][j] as glm indexes, FP32"""
    m = np.asarray(m, F).reshape(4, 4)
    with np.errstate(all="ignore"):
        c00 = m[2, 2] * m[3, 3] - m[3, 2] * m[2, 3]
        c02 = m[1, 2] * m[3, 3] - m[3, 2] * m[1, 3]
        c03 = m[1, 2] * m[2, 3] - m[2, 2] * m[1, 3]
        c04 = m[2, 1] * m[3, 3] - m[3, 1] * m[2, 3]
        c06 = m[1, 1] * m[3, 3] - m[3, 1] * m[1, 3]
        c07 = m[1, 1] * m[2, 3] - m[2, 1] * m[1, 3]
        c08 = m[2, 1] * m[3, 2] - m[3, 1] * m[2, 2]
        c10 = m[1, 1] * m[3, 2] - m[3, 1] * m[1, 2]
        c11 = m[1, 1] * m[2, 2] - m[2, 1] * m[1, 2]
        c12 = m[2, 0] * m[3, 3] - m[3, 0] * m[2, 3]
        c14 = m[1, 0] * m[3, 3] - m[3, 0] * m[1, 3]
        c15 = m[1, 0] * m[2, 3] - m[2, 0] * m[1, 3]
        c16 = m[2, 0] * m[3, 2] - m[3, 0] * m[2, 2]
        c18 = m[1, 0] * m[3, 2] - m[3, 0] * m[1, 2]
        c19 = m[1, 0] * m[2, 2] - m[2, 0] * m[1, 2]
        c20 = m[2, 0] * m[3, 1] - m[3, 0] * m[2, 1]
        c22 = m[1, 0] * m[3, 1] - m[3, 0] * m[1, 1]
        c23 = m[1, 0] * m[2, 1] - m[2, 0] * m[1, 1]
        f0, f1, f2 = np.array([c00, c00, c02, c03], F), np.array([c04, c04, c06, c07], F), np.array([c08, c08, c10, c11], F)
        f3, f4, f5 = np.array([c12, c12, c14, c15], F), np.array([c16, c16, c18, c19], F), np.array([c20, c20, c22, c23], F)
        v0, v1 = np.array([m[1, 0], m[0, 0], m[0, 0], m[0, 0]], F), np.array([m[1, 1], m[0, 1], m[0, 1], m[0, 1]], F)
        v2, v3 = np.array([m[1, 2], m[0, 2], m[0, 2], m[0, 2]], F), np.array([m[1, 3], m[0, 3], m[0, 3], m[0, 3]], F)
        sa, sb = np.array([1, -1, 1, -1], F), np.array([-1, 1, -1, 1], F)
        inv = np.stack([((v1 * f0 - v2 * f1) + v3 * f2) * sa, ((v0 * f0 - v2 * f3) + v3 * f4) * sb,
                        ((v0 * f1 - v1 * f3) + v3 * f5) * sa, ((v0 * f2 - v1 * f4) + v2 * f5) * sb])
        d = m[0] * inv[:, 0]
        dot = (d[0] + d[1]) + (d[2] + d[3])
        out = inv * (F(1.0) / dot)
    assert out.dtype == F
    return out


def glm_mul(a, b):
    """glm's a * b on arrays indexed as glm indexes: r[i][j] = ((a[0][j] b[i][0] + a[1][j] b[i][1]) + a[2][j] b[i][2]) + a[3][j] b[i][3]"""
    a, b = np.asarray(a, F).reshape(4, 4), np.asarray(b, F).reshape(4, 4)
    r = np.zeros((4, 4), F)
    with np.errstate(all="ignore"):
        for i in range(4):
            r[i] = ((a[0] * b[i, 0] + a[1] * b[i, 1]) + a[2] * b[i, 2]) + a[3] * b[i, 3]
    return r


def is_null(R, C):
    return bool((np.asarray(R) == 0).all() and (np.asarray(C) == 0).all())


def transform_cameras(T, fpp, R, C, t):
    """update_camera_transform on copies of the arrays: (R', C', t', P [n, 16]); a null camera is skipped"""
    M = np.asarray(T, np.float64).reshape(4, 4).astype(F)
    fpp = np.asarray(fpp, F).reshape(-1, 3)
    R, C, t = np.array(R, F).reshape(-1, 9), np.array(C, F).reshape(-1, 3), np.array(t, F).reshape(-1, 3)
    P = np.zeros((len(fpp), 16), F)
    inv = glm_inverse(M)
    for v in range(len(fpp)):
        if is_null(R[v], C[v]):
            continue
        E, K = np.zeros((4, 4), F), np.zeros((4, 4), F)
        E[:3, :3], E[:3, 3], E[3, 3] = R[v].reshape(3, 3), t[v], 1
        K[0, 0] = K[1, 1] = fpp[v, 0]
        K[0, 2], K[1, 2], K[2, 2] = fpp[v, 1], fpp[v, 2], 1
        e = glm_mul(inv, E)
        P[v] = glm_mul(e, K).reshape(16)
        R[v], t[v] = e[:3, :3].reshape(9), e[:3, 3]
        C[v] = _point(M, C[v])
    return R, C, t, P


def camera_errors(C, target, null_mask=None):
    """the float accumulator over the non-null cameras, divided by ALL cameras (Q16)"""
    C, target = np.asarray(C, F).reshape(-1, 3), np.asarray(target, np.float64).reshape(-1, 3)
    s = F(0)
    for i in range(len(C)):
        if null_mask is not None and null_mask[i]:
            continue
        d = C[i].astype(np.float64) - target[i]
        s = F(np.float64(s) + np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    return F(s / F(len(C)))
