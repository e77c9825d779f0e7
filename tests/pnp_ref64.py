"""An independent float64 restatement of PnpRansac's contract in numpy, written from the contract's text and not from
tests/pnp_ref.c: the null vector comes from an SVD, the nearest rotation from an SVD, the normal equations from ``numpy.linalg.solve``,
every sum from numpy's own summation.  What it shares with the C file is the integer sampler (tests/epipolar_ref.py's Python mix32).

TEST INFRASTRUCTURE ONLY: numpy alone; nothing under feature_tracker_amd/ may import it.
"""
from __future__ import annotations

import numpy as np

from tests import epipolar_ref as E

SAMPLE = 6


class Result64:
    """R, t (X_cur = R X + t, float64), valid, best, counts [K], kept (bool [n]: the rows that keep TRACKED), participants (indices),
    margin [M] (pixels of reprojection error minus the threshold, +inf behind the camera), steps (accepted refit steps)."""


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


def _errors(c, xy, K):
    """Pixels of reprojection error of camera coordinates c [M, 3] against calibrated xy [M, 2]; +inf where the depth is not positive."""
    with np.errstate(all="ignore"):
        e = np.hypot(K[0] * (c[:, 0] / c[:, 2] - xy[:, 0]), K[1] * (c[:, 1] / c[:, 2] - xy[:, 1]))
    return np.where(c[:, 2] > 0, e, np.inf)


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def solve(landmarks, uv, status, K, hypotheses=512, threshold=1.0, refine_iterations=4, seed=0) -> Result64:
    K = [float(np.float32(k)) for k in K]
    X, uv = np.asarray(landmarks, np.float64), np.asarray(uv, np.float64)
    r = Result64()
    takes = (np.asarray(status) == E.TRACKED) & np.isfinite(X).all(1) & np.isfinite(uv).all(1) & (X != 0).any(1)
    part = np.flatnonzero(takes)
    r.participants, r.valid, r.best, r.counts, r.kept, r.steps = part, -1, -1, np.full(hypotheses, -1), np.zeros(len(X), bool), 0
    r.R, r.t = np.eye(3), np.zeros(3)
    m = len(part)
    if m < SAMPLE:
        return r
    Xp, xy = X[part], np.c_[(uv[part, 0] - K[2]) / K[0], (uv[part, 1] - K[3]) / K[1]]
    Xh = np.c_[Xp, np.ones(m)]
    models = {}
    for h in range(hypotheses):
        idx = _draw(seed, h, m)
        if idx is None:
            continue
        S = Xp[idx]
        mean = S.mean(0)
        s = np.abs(S - mean).mean()
        if not (np.isfinite(s) and s > 0):
            continue
        Sn = np.c_[(S - mean) / s, np.ones(SAMPLE)]
        rows = []
        for (x, y), q in zip(xy[idx], Sn):
            rows += [np.r_[q, np.zeros(4), -x * q], np.r_[np.zeros(4), q, -y * q]]
        A = np.array(rows[:11])
        with np.errstate(all="ignore"):
            if not np.isfinite(A).all():
                continue
            _, sv, Vt = np.linalg.svd(A)
        if sv[-1] <= 1e-9 * sv[0]:  # (rank below 11: the contract's elimination meets a zero pivot)
            continue
        Pn = Vt[-1].reshape(3, 4)
        T = np.eye(4)
        T[:3, :3] /= s
        T[:3, 3] = -mean / s
        Pm = Pn @ T
        w = Pm[2] @ np.c_[S, np.ones(SAMPLE)].T
        if not ((w > 0).all() or (w < 0).all()) or not np.isfinite(Pm).all():
            continue
        if w[0] < 0:
            Pm = -Pm
        models[h] = Pm
        r.counts[h] = int((_errors(Xh @ Pm.T, xy, K) <= threshold).sum())
    if not models:
        return r
    best = int(np.argmax(r.counts))  # (the first maximum: the lowest index among equals)
    A, b = models[best][:, :3], models[best][:, 3]
    U, sv, Vt = np.linalg.svd(A)
    if not (sv[-1] > 0):
        return r
    R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    t = b / sv.mean()
    Rrc, p = R.T, -R.T @ t
    for step in range(refine_iterations):
        c = (Xp - p) @ Rrc
        if step == 0:  # the first step refits on the inliers of the model that won, those in front of the camera under the pose
            inl = (_errors(Xh @ models[best].T, xy, K) <= threshold) & (c[:, 2] > 0)
        else:
            inl = _errors(c, xy, K) <= threshold
        if inl.sum() < SAMPLE:
            break
        ry = K[1] / K[0]
        H, g = np.zeros((6, 6)), np.zeros(6)
        for ci, (x, y) in zip(c[inl], xy[inl]):
            a_, b_, iz = ci[0] / ci[2], ci[1] / ci[2], 1.0 / ci[2]
            Jpi = iz * np.array([[1, 0, -a_], [0, ry, -ry * b_]])
            J = Jpi @ np.c_[_skew(ci), -np.eye(3)]
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
        Rrc, p = Rrc @ (np.eye(3) + _skew(d[:3])), p + Rrc @ d[3:]
        U, _, Vt = np.linalg.svd(Rrc)  # (back onto the rotations: the contract renormalises its quaternion)
        Rrc = U @ Vt
        r.steps += 1
    c = (Xp - p) @ Rrc
    err = _errors(c, xy, K)
    r.margin = err - threshold
    r.kept[part[err <= threshold]] = True
    r.R, r.t, r.valid, r.best = Rrc.T, -Rrc.T @ p, 1, best
    return r
