"""Float64 numpy restatements of what csrc/clip_angles.hip computes, written from the definitions and not from the kernels:

* markley_quat       scipy 1.10.1's Rotation.from_matrix: Markley's quaternion from the RAW matrix, normalised
* procrustes         the nearest rotation U V^T by np.linalg.svd (scipy 1.15.3's first step; the kernel uses a Newton iteration)
* zxy_angles         intrinsic "ZXY" angles of a unit quaternion through its rotation matrix (the kernel goes through the
                     quaternion's half angles), with scipy's rule at the lock
* euler_zxy          both steps, per method;  zxy_matrix: the inverse Rz Rx Ry, for comparing rotations
* smoothing_spline   de Boor's system (6 (1-p) Q^T Q + p R) u = Q^T y, out = y - 6 (1-p) Q u with a DENSE solve up to DENSE_MAX
                     unknowns and a banded L D L^T beyond (tests/test_clip_angles_host.py holds the two to each other)

Everything broadcasts over leading axes; nothing here imports scipy or torch."""
import numpy as np

LOCK = 1e-7          # rad: scipy's gimbal-lock window
DENSE_MAX = 600
METHODS = ("markley", "procrustes")


def markley_branch(m):
    """(..., 3, 3) -> the index of the largest of m00, m11, m22, trace (the first on ties): 0, 1, 2 or 3"""
    m = np.asarray(m, dtype=np.float64)
    d = np.stack([m[..., 0, 0], m[..., 1, 1], m[..., 2, 2], m[..., 0, 0] + m[..., 1, 1] + m[..., 2, 2]], axis=-1)
    return np.argmax(d, axis=-1)


def markley_quat(m):
    """(..., 3, 3) -> (..., 4) unit quaternions (x, y, z, w)"""
    m = np.asarray(m, dtype=np.float64)
    lead = m.shape[:-2]
    m = m.reshape(-1, 3, 3)
    choice = markley_branch(m)
    tr = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
    q = np.empty((m.shape[0], 4))
    for n in range(m.shape[0]):
        i = int(choice[n])
        if i == 3:
            q[n] = (m[n, 2, 1] - m[n, 1, 2], m[n, 0, 2] - m[n, 2, 0], m[n, 1, 0] - m[n, 0, 1], 1.0 + tr[n])
        else:
            j, k = (i + 1) % 3, (i + 2) % 3
            q[n, i] = 1.0 - tr[n] + 2.0 * m[n, i, i]
            q[n, j] = m[n, j, i] + m[n, i, j]
            q[n, k] = m[n, k, i] + m[n, i, k]
            q[n, 3] = m[n, k, j] - m[n, j, k]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.reshape(lead + (4,))


def procrustes(m):
    """(..., 3, 3) with positive determinant -> the nearest rotation"""
    u, _, vt = np.linalg.svd(np.asarray(m, dtype=np.float64))
    return u @ vt


def quat_matrix(q):
    x, y, z, w = (q[..., i] for i in range(4))
    r = np.empty(q.shape[:-1] + (3, 3))
    r[..., 0, 0] = 1 - 2 * (y * y + z * z)
    r[..., 0, 1] = 2 * (x * y - z * w)
    r[..., 0, 2] = 2 * (x * z + y * w)
    r[..., 1, 0] = 2 * (x * y + z * w)
    r[..., 1, 1] = 1 - 2 * (x * x + z * z)
    r[..., 1, 2] = 2 * (y * z - x * w)
    r[..., 2, 0] = 2 * (x * z - y * w)
    r[..., 2, 1] = 2 * (y * z + x * w)
    r[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return r


def zxy_angles(q):
    """unit quaternions (..., 4) -> (..., 3) degrees (Z, X, Y), R = Rz(Z) Rx(X) Ry(Y):
        R = [[cz cy - sz sx sy, -sz cx, cz sy + sz sx cy], [sz cy + cz sx sy, cz cx, sz sy - cz sx cy], [-cx sy, sx, cx cy]]
    so X = atan2(R21, |(R20, R22)|), Z = atan2(-R01, R11), Y = atan2(-R20, R22); where cx = |(R20, R22)| <= sin(LOCK), Y = 0 and
    Z = atan2(R10, R00), the combined rotation (cos and sin of Z + Y at X = 90 degrees, of Z - Y at X = -90 degrees)."""
    r = quat_matrix(np.asarray(q, dtype=np.float64))
    cx = np.hypot(r[..., 2, 0], r[..., 2, 2])
    lock = cx <= np.sin(LOCK)
    X = np.arctan2(r[..., 2, 1], cx)
    Z = np.where(lock, np.arctan2(r[..., 1, 0], r[..., 0, 0]), np.arctan2(-r[..., 0, 1], r[..., 1, 1]))
    Y = np.where(lock, 0.0, np.arctan2(-r[..., 2, 0], r[..., 2, 2]))
    return np.degrees(np.stack([Z, X, Y], axis=-1))


def euler_zxy(m, method):
    """(..., 3, 3) raw matrices -> (..., 3) degrees; a matrix whose determinant is not > 0 gives NaN"""
    assert method in METHODS
    m = np.asarray(m, dtype=np.float64)
    bad = ~(np.linalg.det(m) > 0)
    safe = np.where(bad[..., None, None], np.eye(3), m)
    out = zxy_angles(markley_quat(procrustes(safe) if method == "procrustes" else safe))
    out[bad] = np.nan
    return out


def zxy_matrix(angles_deg):
    """(..., 3) degrees (Z, X, Y) -> (..., 3, 3) Rz(Z) Rx(X) Ry(Y)"""
    a = np.radians(np.asarray(angles_deg, dtype=np.float64))
    cz, sz, cx, sx, cy, sy = np.cos(a[..., 0]), np.sin(a[..., 0]), np.cos(a[..., 1]), np.sin(a[..., 1]), np.cos(a[..., 2]), np.sin(a[..., 2])
    r = np.empty(a.shape[:-1] + (3, 3))
    r[..., 0, 0] = cz * cy - sz * sx * sy
    r[..., 0, 1] = -sz * cx
    r[..., 0, 2] = cz * sy + sz * sx * cy
    r[..., 1, 0] = sz * cy + cz * sx * sy
    r[..., 1, 1] = cz * cx
    r[..., 1, 2] = sz * sy - cz * sx * cy
    r[..., 2, 0] = -cx * sy
    r[..., 2, 1] = sx
    r[..., 2, 2] = cx * cy
    return r


def frames_to_angles(frames, method):
    """(..., 9 J) -> (..., 3 J): the layout of g2v_rotmat_to_euler"""
    frames = np.asarray(frames, dtype=np.float64)
    J = frames.shape[-1] // 9
    return euler_zxy(frames.reshape(frames.shape[:-1] + (J, 3, 3)), method).reshape(frames.shape[:-1] + (3 * J,))


def angle_diff(a, b):
    """|a - b| modulo 360 degrees"""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)


def spline_bands(p):
    """the pentadiagonal Toeplitz matrix 6 (1-p) Q^T Q + p R as (a0, a1, a2): diagonal, first and second off-diagonal"""
    k = 6.0 * (1.0 - p)
    return 6.0 * k + 4.0 * p, -4.0 * k + p, k


def _solve_dense(n, bands, rhs):
    a0, a1, a2 = bands
    A = a0 * np.eye(n) + a1 * (np.eye(n, k=1) + np.eye(n, k=-1)) + a2 * (np.eye(n, k=2) + np.eye(n, k=-2))
    return np.linalg.solve(A, rhs)


def _solve_banded(n, bands, rhs):
    """L D L^T of bandwidth 2, then the two substitutions; rhs (n, columns)"""
    a0, a1, a2 = bands
    d, e, f = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        f[i] = a2 / d[i - 2] if i >= 2 else 0.0
        e[i] = (a1 - (f[i] * e[i - 1] * d[i - 2] if i >= 2 else 0.0)) / d[i - 1] if i >= 1 else 0.0
        d[i] = a0 - (e[i] ** 2 * d[i - 1] if i >= 1 else 0.0) - (f[i] ** 2 * d[i - 2] if i >= 2 else 0.0)
    z = np.array(rhs, dtype=np.float64)
    for i in range(n):
        if i >= 1:
            z[i] -= e[i] * z[i - 1]
        if i >= 2:
            z[i] -= f[i] * z[i - 2]
    z /= d[:, None]
    for i in range(n - 1, -1, -1):
        if i + 1 < n:
            z[i] -= e[i + 1] * z[i + 1]
        if i + 2 < n:
            z[i] -= f[i + 2] * z[i + 2]
    return z


def smoothing_spline(y, p, axis=0, solver=None):
    """the cubic smoothing spline of y along `axis` at unit-spaced knots, csaps' smoothing parameter p in [0, 1]"""
    y = np.moveaxis(np.asarray(y, dtype=np.float64), axis, 0)
    F = y.shape[0]
    flat = y.reshape(F, -1)
    n = F - 2
    if n < 1 or p == 1.0:
        out = flat.copy()
    else:
        rhs = flat[:-2] - 2.0 * flat[1:-1] + flat[2:]
        solve = solver or (_solve_dense if n <= DENSE_MAX else _solve_banded)
        u = solve(n, spline_bands(p), rhs)
        qu = np.zeros_like(flat)
        qu[:-2] += u
        qu[1:-1] -= 2.0 * u
        qu[2:] += u
        out = flat - 6.0 * (1.0 - p) * qu
    return np.moveaxis(out.reshape(y.shape), 0, axis)


# ---- the inputs the tests and the fixture script share ---------------------------------------------------------------------------
NOISE = 0.05
X_MAX_DRAW, X_MAX_HELD = 70.0, 80.0


def noisy_matrices(n, seed):
    """n float32 matrices: Rz Rx Ry of angles with X uniform in [-70, 70] degrees and Z, Y in [-180, 180], plus Gaussian noise of
    0.05 on every entry (the issue's condition for the angle-by-angle comparison)"""
    rng = np.random.RandomState(seed)
    ang = np.stack([rng.uniform(-180, 180, n), rng.uniform(-X_MAX_DRAW, X_MAX_DRAW, n), rng.uniform(-180, 180, n)], axis=-1)
    return (zxy_matrix(ang) + NOISE * rng.standard_normal((n, 3, 3))).astype(np.float32)


def branch_matrices():
    """float64 exact rotations that reach every Markley branch: turns by 179 and 180 degrees about x, y and z (branches 0, 1, 2)
    and small turns (branch 3, the trace) -> (12, 3, 3), as (Z, X, Y) angles put through zxy_matrix"""
    ang = [(0, 0, 0), (3, -2, 5), (20, 10, -15), (-35, 25, 30),            # trace
           (180, 0, 180), (179, 1, 180), (-178, 2, 179),                   # about x: Rz(180) Ry(180) = Rx(180)
           (0, 0, 180), (1, 2, 179), (2, -1, -178),                        # about y
           (180, 0, 0), (179, 1, 2)]                                       # about z
    return zxy_matrix(np.array(ang, dtype=np.float64))


def spline_data(F, cols, seed):
    """(F, cols) float32 within [-180, 180]: a slow wave plus noise, one column a straight line, one a constant"""
    rng = np.random.RandomState(seed)
    t = np.arange(F, dtype=np.float64)[:, None]
    y = 90.0 * np.sin(2 * np.pi * t / max(F, 8) * rng.uniform(0.5, 3.0, cols) + rng.uniform(0, 6, cols)) + 40.0 * rng.standard_normal((F, cols))
    if cols > 1:
        y[:, 1] = np.linspace(-170.0, 175.0, F)
    if cols > 2:
        y[:, 2] = 33.25
    return np.clip(y, -180.0, 180.0).astype(np.float32)
