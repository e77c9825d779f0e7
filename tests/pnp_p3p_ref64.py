"""An independent float64 statement of PnpRansac's "p3p" sampler in numpy, written from the contract's text and not from
tests/pnp_p3p_ref.c.  The P3P solutions come by another route than the restatement's: the quartic is the one in s1 / s0 (the restatement
eliminates down to s2 / s0), its coefficients come from numpy's polynomial products, its roots from ``numpy.roots`` (the companion
matrix), and the pose of a solution from an SVD (Kabsch) on the three points instead of two frames.  The helpers of the other stages
are tests/pnp_ref64.py's; what it shares with the C file is the integer sampler.

TEST INFRASTRUCTURE ONLY: numpy alone; nothing under feature_tracker_amd/ may import it.
"""
from __future__ import annotations

import numpy as np

from tests import epipolar_ref as E
from tests import pnp_ref64 as R64

SAMPLE, REFIT_MIN = 4, 6
IMAGINARY = 1e-7  # a root of numpy.roots counts as real below this imaginary part


def p3p(xy, X):
    """Calibrated pixels [3, 2] and landmarks [3, 3] -> (solutions [(R, t)], gap): every real solution with three positive distances, and the
    least distance between two roots of the quartic (a count is only comparable where the roots stand apart).  None: degenerate."""
    xy, X = np.asarray(xy, np.float64), np.asarray(X, np.float64)
    f = np.c_[xy, np.ones(3)]
    f /= np.linalg.norm(f, axis=1)[:, None]
    if not (np.isfinite(f).all() and np.isfinite(X).all()):
        return None
    if np.linalg.norm(np.cross(X[1] - X[0], X[2] - X[0])) <= 0 or min(np.linalg.norm(np.cross(f[i], f[j])) for i, j in ((0, 1), (0, 2), (1, 2))) <= 0:
        return None
    c01, c02, c12 = f[0] @ f[1], f[0] @ f[2], f[1] @ f[2]
    d01, d02, d12 = (np.sum((X[j] - X[i]) ** 2) for i, j in ((0, 1), (0, 2), (1, 2)))
    # s1 = u s0, s2 = v s0: (1 + u^2 - 2 u c01) d02 = (1 + v^2 - 2 v c02) d01 and (u^2 + v^2 - 2 u v c12) d01 = (1 + u^2 - 2 u c01) d12.
    # Their combination without v^2 is linear in v: v = N(u) / D(u); polynomials in u, highest power first.
    q = np.array([1.0, -2 * c01, 1.0])                              # 1 + u^2 - 2 u c01
    N = np.polysub(np.polymul([(d02 - d12) / d01], q), [-1.0, 0.0, 1.0])   # ((d02 - d12) / d01) q - (1 - u^2)
    D = np.array([2 * c12, -2 * c02])                               # 2 (c12 u - c02)
    # into the second equation times D^2: N^2 + u^2 D^2 - 2 c12 u N D - (d12 / d01) q D^2 = 0
    D2 = np.polymul(D, D)
    quartic = np.polyadd(np.polymul(N, N), np.polymul([1.0, 0.0, 0.0], D2))
    quartic = np.polysub(quartic, 2 * c12 * np.polymul([1.0, 0.0], np.polymul(N, D)))
    quartic = np.polysub(quartic, d12 / d01 * np.polymul(q, D2))
    roots = np.roots(quartic)
    gap = min([abs(a - b) for i, a in enumerate(roots) for b in roots[i + 1:]], default=np.inf)
    out = []
    for root in roots:
        if abs(root.imag) > IMAGINARY:
            continue
        u = root.real
        v = np.polyval(N, u) / np.polyval(D, u)
        if not (np.isfinite(v) and u > 0 and v > 0):
            continue
        s0 = np.sqrt(d01 / np.polyval(q, u))
        Y = np.array([s0, u * s0, v * s0])[:, None] * f
        # Kabsch: the rotation that takes the centred landmarks onto the centred camera points
        Xc, Yc = X - X.mean(0), Y - Y.mean(0)
        U, _, Vt = np.linalg.svd(Yc.T @ Xc)
        Rm = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
        out.append((Rm, Y.mean(0) - Rm @ X.mean(0)))
    return out, gap


def _draw(seed, h, m):
    idx = []
    for k in range(SAMPLE):
        for a in range(E.ATTEMPTS):
            j = (E.mix32(seed & 0xFFFFFFFF, h, k, a) * m) >> 32
            if j not in idx:
                idx.append(j)
                break
        else:
            return None
    return idx


def solve(landmarks, uv, status, K, hypotheses=512, threshold=1.0, refine_iterations=4, seed=0) -> R64.Result64:
    """pnp_ref64.solve under the "p3p" sampler: a Result64."""
    K = [float(np.float32(k)) for k in K]
    X, uv = np.asarray(landmarks, np.float64), np.asarray(uv, np.float64)
    r = R64.Result64()
    takes = (np.asarray(status) == E.TRACKED) & np.isfinite(X).all(1) & np.isfinite(uv).all(1) & (X != 0).any(1)
    part = np.flatnonzero(takes)
    r.participants, r.valid, r.best, r.counts, r.kept, r.steps = part, -1, -1, np.full(hypotheses, -1), np.zeros(len(X), bool), 0
    r.R, r.t = np.eye(3), np.zeros(3)
    m = len(part)
    if m < SAMPLE:
        return r
    Xp, xy = X[part], np.c_[(uv[part, 0] - K[2]) / K[0], (uv[part, 1] - K[3]) / K[1]]
    ry = K[1] / K[0]
    models = {}
    for h in range(hypotheses):
        idx = _draw(seed, h, m)
        if idx is None:
            continue
        found = p3p(xy[idx[:3]], Xp[idx[:3]])
        best = None
        for Rm, t in (found[0] if found else []):
            c = Xp[idx] @ Rm.T + t
            if not (c[:, 2] > 0).all():
                continue
            err = (c[3, 0] - xy[idx[3], 0] * c[3, 2]) ** 2 + ((c[3, 1] - xy[idx[3], 1] * c[3, 2]) * ry) ** 2
            if np.isfinite(err) and (best is None or err < best[0]):
                best = (err, np.c_[Rm, t])
        if best is None:
            continue
        models[h] = best[1]
        r.counts[h] = int((R64._errors(Xp @ best[1][:, :3].T + best[1][:, 3], xy, K) <= threshold).sum())
    if not models:
        return r
    best = int(np.argmax(r.counts))
    R, t = models[best][:, :3], models[best][:, 3]
    Rrc, p = R.T, -R.T @ t
    for step in range(refine_iterations):
        c = (Xp - p) @ Rrc
        if step == 0:
            inl = (R64._errors(Xp @ R.T + t, xy, K) <= threshold) & (c[:, 2] > 0)
        else:
            inl = R64._errors(c, xy, K) <= threshold
        if inl.sum() < REFIT_MIN:
            break
        H, g = np.zeros((6, 6)), np.zeros(6)
        for ci, (x, y) in zip(c[inl], xy[inl]):
            a_, b_, iz = ci[0] / ci[2], ci[1] / ci[2], 1.0 / ci[2]
            J = iz * np.array([[1, 0, -a_], [0, ry, -ry * b_]]) @ np.c_[R64._skew(ci), -np.eye(3)]
            res = np.array([a_ - x, (b_ - y) * ry])
            H += J.T @ J
            g += J.T @ res
        try:
            np.linalg.cholesky(H)
            d = np.linalg.solve(H, -g)
        except np.linalg.LinAlgError:
            break
        if not np.isfinite(d).all():
            break
        Rrc, p = Rrc @ (np.eye(3) + R64._skew(d[:3])), p + Rrc @ d[3:]
        U, _, Vt = np.linalg.svd(Rrc)
        Rrc = U @ Vt
        r.steps += 1
    err = R64._errors((Xp - p) @ Rrc, xy, K)
    r.margin = err - threshold
    r.kept[part[err <= threshold]] = True
    r.R, r.t, r.valid, r.best = Rrc.T, -Rrc.T @ p, 1, best
    return r
