"""ref64 for DirectMethod: a float64 restatement of the reference's direct_method_tracker.cpp / .h (photometric Gauss-Newton on one
6-DoF pose over all features jointly).

TEST INFRASTRUCTURE ONLY.  Written from the reference's source and DESIGN.md §2's substrate table (GetPixelValue validity and
bilinear sampling, CameraPinhole::LiftFromNormalizedPlaneToImagePlane as u = fx x + cx, kZeroFloat = 1e-6), independently of the C
restatement the GPU tests compare against bit for bit: it imports numpy, the standard library and the substrate helper
tests.klt_ref64._Image (itself independent), and shares no line with that restatement or with the package.

Precision rule (as in klt_ref64): every sample coordinate is formed in float32 exactly as the reference forms it
(`static_cast<float>(drow) + uv.y()`, `col_j - 1.0f`, `ref_pixel_uv / scale`, `*= 2.0f`) from the float32 rounding of the carried
cur_pixel_uv, so validity decisions are the reference's own; the `p_r_z < kZeroFloat` test is made on the float32 input.
Everything else is float64: quaternions by the textbook formulas (q * v as v + 2 w (u x v) + 2 u x (u x v), which is what Eigen
evaluates also for a quaternion that is not of unit length; the inverse as conjugate / squared norm), projection, Jacobian, taps,
products, sums, numpy.linalg.solve, the update, and the state carried over iterations and levels.

Two facts of the source that a test has to handle are visible in the Result:
* `uv[i]` is written at the START of an iteration, from the pose that iteration starts with (:141-145): after the last iteration
  it lags the returned pose (q, p) by one update.  `project()` gives the pixels a pose induces.
* `uv[i]` is written only for points that pass both z tests (:130, :142); `written[i]` is False for a point that never did, and
  its uv is the incoming value, bit for bit.

Besides pose, pixels, status and the total iteration count the Result reports what a test needs to decide comparability:
* `m_converge`  smallest | |dx|^2 - kMaxConvergeStep | / kMaxConvergeStep over the convergence tests taken;
* `m_z`         smallest |z - kZeroFloat| over the tested z of points in the CURRENT frame (computed values; the test on the
                float32 input z is exact and shared with any faithful implementation, so it carries no margin);
* `m_outside`   per feature, the px distance of the final pixel to the outside bounds (inf for a pixel never written: an input);
* `m_edge`      smallest px distance of a current-image sample to a validity edge (reported, does not gate: one flipped sample
                among tens of thousands of terms does not move the pose measurably);
* `cond`        the largest 2-norm condition number of a solved H; `singular`: a solved H had rank below 6 (solved by
                pseudo-inverse; Eigen's zero-pivot rule decides such a step, so it is not comparable);
* `capped`      a level ran out of iterations without a stopping decision.

`Flags` carries the negative-control mutations the tests use to show that they can fail.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from tests.klt_ref64 import _Image

NOT_TRACKED, TRACKED, LARGE_RESIDUAL, OUTSIDE, NUMERIC_ERROR = range(5)  # feature_tracker.h TrackStatus

f32 = np.float32
K_ZERO = float(f32(1e-6))  # kZeroFloat


@dataclasses.dataclass(frozen=True)
class Flags:
    """Mutations, each off by default (swap_sr_sc and validity_strict are read by klt_ref64._Image)."""
    swap_sr_sc: bool = False                 # bilinear row / column fractions swapped
    validity_strict: bool = False
    no_half_gradient: bool = False           # central difference without * 0.5 (:166)
    jacobian_at_current_point: bool = False  # the 2x6 Jacobian at p_c_in_cur instead of p_c_in_ref (:149-151)
    flip_rotation_column: int = -1           # sign of Jacobian column 3, 4 or 5
    swap_columns_3_4: bool = False
    update_on_the_right: bool = False        # q_rc * dq instead of dq * q_rc (:184)
    no_inverse: bool = False                 # q_rc instead of q_rc.inverse() in the projection (:141)
    principal_point_not_scaled: bool = False  # cx, cy kept at level 0's value on every level (:53, :68-70)
    uv_from_updated_pose: bool = False       # cur_pixel_uv written after the update
    converge_on_translation_only: bool = False  # dx.head<3>().squaredNorm() in the convergence test (:188)
    outside_inclusive: bool = False          # kOutside tested with <= / >= (:79-80)


DEFAULT = Flags()


@dataclasses.dataclass(frozen=True)
class Options:  # direct_method_tracker.h:20-28
    kMaxTrackPointsNumber: int = 500
    kMaxIteration: int = 15
    kPatchRowHalfSize: int = 6
    kPatchColHalfSize: int = 6
    kMaxConvergeStep: float = 1e-6
    kMethod: str = "direct"  # "inverse" and "fast" are empty stubs (:108-113, :194-199)


@dataclasses.dataclass
class Result:
    ok: bool
    uv: np.ndarray        # (n, 2) float64
    q: np.ndarray         # (4,) w, x, y, z
    p: np.ndarray         # (3,)
    status: np.ndarray    # (n,) uint8
    iters: int
    written: np.ndarray   # (n,) bool
    m_converge: float = np.inf
    m_z: float = np.inf
    m_outside: np.ndarray = None
    m_edge: float = np.inf
    cond: float = 0.0
    singular: bool = False
    capped: bool = False
    solved: int = 0


# ---- quaternions (w, x, y, z), float64 --------------------------------------------------------------------------------------------

def q_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw])


def q_inverse(q):
    n2 = float(np.dot(q, q))
    if not n2 > 0.0:
        return np.zeros(4)
    return np.array([q[0], -q[1], -q[2], -q[3]]) / n2


def q_normalized(q):
    n2 = float(np.dot(q, q))
    return q / np.sqrt(n2) if n2 > 0.0 else q


def q_matrix(q):
    """The linear map of Eigen's `q * v`: I + 2 w [u]x + 2 [u]x^2 (a rotation iff |q| = 1)."""
    w, x, y, z = q
    S = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + 2.0 * w * S + 2.0 * (S @ S)


def q_rotate(q, v):
    return np.asarray(v, np.float64) @ q_matrix(q).T


def project(K, q_rc, p_rc, points):
    """Pixels of reference-frame `points` in the frame of pose (q_rc, p_rc): K (q_rc^-1 (X - p_rc)), float64; (pixels, z)."""
    fx, fy, cx, cy = (float(k) for k in K)
    pc = (np.asarray(points, np.float64) - np.asarray(p_rc, np.float64)) @ q_matrix(q_inverse(np.asarray(q_rc, np.float64))).T
    z = pc[:, 2]
    return np.stack([fx * pc[:, 0] / z + cx, fy * pc[:, 1] / z + cy], 1), z


def grid_points(K, rows, cols, depths, step=40):
    """Reference-frame points behind a pixel grid spanning the image, at each of `depths`."""
    fx, fy, cx, cy = (float(k) for k in K)
    us, vs = np.meshgrid(np.arange(0, cols, step, dtype=np.float64), np.arange(0, rows, step, dtype=np.float64))
    out = []
    for z in depths:
        out.append(np.stack([(us.ravel() - cx) / fx * z, (vs.ravel() - cy) / fy * z, np.full(us.size, float(z))], 1))
    return np.concatenate(out)


# ---- TrackAllFeaturesDirect (:115-192) ----------------------------------------------------------------------------------------------

def _jacobian(X, fx, fy, fl):
    """d pixel / d xi at the points X (m, 3): (m, 2, 6), columns 0-2 translation, 3-5 rotation (:148-151)."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    zi = 1.0 / z
    zi2 = zi * zi
    J = np.zeros((len(X), 2, 6))
    J[:, 0, 0] = fx * zi
    J[:, 0, 2] = -fx * x * zi2
    J[:, 0, 3] = -fx * x * y * zi2
    J[:, 0, 4] = fx + fx * x * x * zi2
    J[:, 0, 5] = -fx * y * zi
    J[:, 1, 1] = fy * zi
    J[:, 1, 2] = -fy * y * zi2
    J[:, 1, 3] = -fy - fy * y * y * zi2
    J[:, 1, 4] = fy * x * y * zi2
    J[:, 1, 5] = fy * x * zi
    if fl.flip_rotation_column >= 0:
        J[:, :, fl.flip_rotation_column] *= -1.0
    if fl.swap_columns_3_4:
        J[:, :, [3, 4]] = J[:, :, [4, 3]]
    return J


def normal_equations(refI, curI, K, pts, ref32, uv, q, p, o, fl, report=None):
    """One iteration's H and b (:124-176) at the pose (q, p).  Writes uv (float64, in place) for the points that pass both z tests
    and returns (H, b, ids of those points)."""
    fx, fy, cx, cy = K
    m = min(len(ref32), int(o.kMaxTrackPointsNumber))
    keep = ~(pts[:m, 2] < f32(1e-6))  # :130, on the float32 input
    P = pts[:m].astype(np.float64)
    M = q_matrix(q if fl.no_inverse else q_inverse(q))
    pc = (P - p) @ M.T
    z = pc[:, 2]
    if report is not None and keep.any():
        report["m_z"] = min(report["m_z"], float(np.abs(z[keep] - K_ZERO).min()))
    with np.errstate(invalid="ignore"):
        ids = np.nonzero(keep & ~(z < K_ZERO))[0]  # :142
    H, b = np.zeros((6, 6)), np.zeros(6)
    if len(ids) == 0:
        return H, b, ids
    uv[ids, 0] = fx * (pc[ids, 0] / z[ids]) + cx  # :144-145
    uv[ids, 1] = fy * (pc[ids, 1] / z[ids]) + cy
    J = _jacobian(pc[ids] if fl.jacobian_at_current_point else P[ids], fx, fy, fl)
    hr, hc = int(o.kPatchRowHalfSize), int(o.kPatchColHalfSize)
    drow, dcol = np.meshgrid(np.arange(-hr, hr + 1), np.arange(-hc, hc + 1), indexing="ij")
    drow, dcol = f32(drow.ravel())[None, :], f32(dcol.ravel())[None, :]
    cur32 = uv[ids].astype(f32)
    r32 = ref32[ids]
    row_i, col_i = drow + r32[:, 1:2], dcol + r32[:, 0:1]  # :157-160, float32
    row_j, col_j = drow + cur32[:, 1:2], dcol + cur32[:, 0:1]
    one = f32(1.0)
    edge = report is not None
    with np.errstate(invalid="ignore", over="ignore"):
        t0, v0, e0 = curI.get(row_j, col_j - one, fl, edge)
        t1, v1, e1 = curI.get(row_j, col_j + one, fl, edge)
        t2, v2, e2 = curI.get(row_j - one, col_j, fl, edge)
        t3, v3, e3 = curI.get(row_j + one, col_j, fl, edge)
        t4, v4, _ = refI.get(row_i, col_i, fl, False)
        t5, v5, e5 = curI.get(row_j, col_j, fl, edge)
    valid = v0 & v1 & v2 & v3 & v4 & v5
    if edge:
        report["m_edge"] = min(report["m_edge"], float(np.min([e.min() for e in (e0, e1, e2, e3, e5)])))
    g = 1.0 if fl.no_half_gradient else 0.5
    gx = np.where(valid, (t1 - t0) * g, 0.0)
    gy = np.where(valid, (t3 - t2) * g, 0.0)
    res = np.where(valid, t5 - t4, 0.0)
    jac = gx[:, :, None] * J[:, None, 0, :] + gy[:, :, None] * J[:, None, 1, :]  # (m, patch, 6), :170
    H = np.einsum("mpi,mpj->ij", jac, jac)
    b = np.einsum("mp,mpi->i", res, jac)
    return H, b, ids


def _solve(H, b, report):
    if not (np.isfinite(H).all() and np.isfinite(b).all()):
        return np.full(6, np.nan)
    sv = np.linalg.svd(H, compute_uv=False)
    report["solved"] += 1
    if not (sv[0] > 0.0 and sv[-1] > sv[0] * 1e-13):
        report["singular"] = True
        return np.linalg.pinv(H) @ b
    report["cond"] = max(report["cond"], float(sv[0] / sv[-1]))
    return np.linalg.solve(H, b)


def _track_level(refI, curI, K, pts, ref32, uv, written, q, p, o, fl, report):
    thr = float(f32(o.kMaxConvergeStep))
    for _ in range(int(o.kMaxIteration)):
        report["iters"] += 1
        H, b, ids = normal_equations(refI, curI, K, pts, ref32, uv, q, p, o, fl, report)
        written[ids] = True
        dx = _solve(H, b, report)
        if np.isnan(dx).any():  # :180
            return q, p
        p = p + dx[:3]
        dq = q_normalized(np.array([1.0, 0.5 * dx[3], 0.5 * dx[4], 0.5 * dx[5]]))
        q = q_normalized(q_mul(q, dq) if fl.update_on_the_right else q_mul(dq, q))  # :184-185
        if fl.uv_from_updated_pose and len(ids):
            px, z = project(K, q, p, pts[ids].astype(np.float64))
            uv[ids] = px
        sq = float(np.dot(dx[:3], dx[:3]) if fl.converge_on_translation_only else np.dot(dx, dx))
        report["m_converge"] = min(report["m_converge"], abs(sq - thr) / thr)
        if sq < thr:  # :188
            return q, p
    report["capped"] = True
    return q, p


# ---- TrackFeatures, camera-frame overload (:35-86) --------------------------------------------------------------------------------

def _options(method, half, half_cols, max_points, max_iteration, converge):
    return Options(int(max_points), int(max_iteration), int(half), int(half if half_cols is None else half_cols), float(converge), method)


def track(ref_levels, cur_levels, K, p_c_in_ref, ref_uv, cur_uv=None, q_rc=(1, 0, 0, 0), p_rc=(0, 0, 0), status=None, *, method="direct",
          half=6, half_cols=None, max_points=500, max_iteration=15, converge=1e-6, flags=DEFAULT, _pose64=None):
    """TrackFeatures(ref_pyramid, cur_pyramid, K, p_c_in_ref, ref_pixel_uv, cur_pixel_uv, q_rc, p_rc, status): a Result.
    (_pose64: the world-frame overload's start pose, which keeps its float64 value.)"""
    o = _options(method, half, half_cols, max_points, max_iteration, converge)
    ref = np.asarray(ref_uv, np.float32).reshape(-1, 2)
    n = len(ref)
    q = np.asarray(q_rc, np.float32).astype(np.float64).reshape(4)
    p = np.asarray(p_rc, np.float32).astype(np.float64).reshape(3)
    if _pose64 is not None:
        q, p = _pose64
    pts = np.asarray(p_c_in_ref, np.float32).reshape(-1, 3)
    given = cur_uv is not None and np.asarray(cur_uv).reshape(-1, 2).shape[0] == n
    uv = (np.asarray(cur_uv, np.float32).reshape(-1, 2) if given else ref).astype(np.float64)  # :42-44
    st_valid = status is not None and np.asarray(status).size == n
    st = np.asarray(status, np.uint8).copy() if st_valid else np.zeros(n, np.uint8)
    written = np.zeros(n, bool)
    if n == 0 or len(ref_levels) != len(cur_levels):  # :38-39
        return Result(False, uv, q, p, st, 0, written, m_outside=np.full(n, np.inf))
    L = len(ref_levels)
    report = dict(iters=0, m_converge=np.inf, m_z=np.inf, m_edge=np.inf, cond=0.0, singular=False, capped=False, solved=0)
    scale = f32(1 << (L - 1))
    sref = ref / scale  # :51, float32
    Kf = np.asarray(K, np.float32).reshape(4)
    sK = Kf / scale  # :53
    for lvl in range(L - 1, -1, -1):
        if o.kMethod == "direct":
            Kl = sK.astype(np.float64)
            if flags.principal_point_not_scaled:
                Kl[2:] = Kf[2:].astype(np.float64)
            q, p = _track_level(_Image(ref_levels[lvl]), _Image(cur_levels[lvl]), Kl, pts, sref, uv, written, q, p, o, flags, report)
        if lvl == 0:
            break
        sref = sref * f32(2.0)  # :66
        sK = sK * f32(2.0)      # :69
    if not st_valid:  # :74-76
        st[:] = TRACKED
    rows, cols = np.asarray(ref_levels[0]).shape
    x, y = uv[:, 0], uv[:, 1]
    with np.errstate(invalid="ignore"):
        if flags.outside_inclusive:
            out = (x <= 0) | (x >= cols - 1) | (y <= 0) | (y >= rows - 1)
        else:
            out = (x < 0) | (x > cols - 1) | (y < 0) | (y > rows - 1)  # :79-80
        margin = np.minimum(np.minimum(np.abs(x), np.abs(x - (cols - 1))), np.minimum(np.abs(y), np.abs(y - (rows - 1))))
    st[out] = OUTSIDE
    return Result(True, uv, q, p, st, report["iters"], written, report["m_converge"], report["m_z"], np.where(written, margin, np.inf),
                  report["m_edge"], report["cond"], report["singular"], report["capped"], report["solved"])


# ---- TrackFeatures, world-frame overload (:8-33) ------------------------------------------------------------------------------------

def track_world(ref_levels, cur_levels, K, ref_q_wc, ref_p_wc, p_w, ref_uv, cur_uv=None, cur_q_wc=(1, 0, 0, 0), cur_p_wc=(0, 0, 0), status=None,
                **kw):
    """The Result's (q, p) is the current frame's world pose.  The lifted points are handed on as float32, the type of the
    reference's p_c_in_ref_, so that the camera-frame overload's z test sees the values the reference's sees (up to their rounding)."""
    rq = np.asarray(ref_q_wc, np.float32).astype(np.float64)
    rp = np.asarray(ref_p_wc, np.float32).astype(np.float64)
    cq = np.asarray(cur_q_wc, np.float32).astype(np.float64)
    cp = np.asarray(cur_p_wc, np.float32).astype(np.float64)
    r_cw = q_inverse(rq)
    pw = np.asarray(p_w, np.float32).reshape(-1, 3).astype(np.float64)
    p_c = q_rotate(r_cw, pw - rp)
    q_rc = q_mul(r_cw, cq)
    p_rc = q_rotate(r_cw, cp - rp)
    r = track(ref_levels, cur_levels, K, p_c, ref_uv, cur_uv, status=status, _pose64=(q_rc, p_rc), **kw)
    if not r.ok:
        r.q, r.p = cq, cp
        return r
    r.q, r.p = q_mul(rq, r.q), q_rotate(rq, r.p) + rp
    return r
