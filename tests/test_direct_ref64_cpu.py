"""DirectMethod's oracle against ref64 (tests/direct_ref64.py), a float64 restatement of direct_method_tracker.cpp written
independently of oracle/oracle_direct_method.c, at the north-star bar (1e-3 px, BASELINE.json); the kernels directly in
tests/test_direct_ref64_gpu.py, which shares the cases and the criterion below.

Criterion (check()), none of it taken from the code under test:
* `ok`, every status and - wherever ref64's m_converge is outside BAND_REL and no level ran out of iterations - the iteration count
  are equal;
* every pixel ref64 wrote agrees within TOL_PX; a pixel ref64 never wrote (its point failed a z test) equals its input bit for bit;
* the POSE agrees through the pixels it induces: a grid spanning the image, lifted to the scene's nearest and farthest depth, is
  projected with ref64's pose and with the pose under test; the largest displacement is at most TOL_PX.  (cur_pixel_uv lags the
  returned pose by one update, so the pixels alone would not see a wrong final update.)
Every committed case must be comparable by ref64's own report: not singular, m_converge > BAND_REL, m_z > BAND_Z, m_outside >=
BAND_PX for every written pixel.  The exceptions are named in DEGENERATE and are degenerate on purpose: the textureless image and
the all-points-skipped problem (H = 0, so dx = 0 under any solver: ref64's pose is the start pose, a test asserts that, and ok,
status, iterations and "nothing moved" - pixels and induced pixels against that pose - are compared), and, beyond the two the issue
names, the single-feature problem: three features capped to one.  One feature's terms span at most two directions of the six, so H
has rank <= 2 whatever the image, and Eigen's zero-pivot rule, not the reference's source, decides its steps, iteration count and
the tracked feature's final status.  What does not depend on the solver is compared: ok, the sizes, that the two features beyond
the cap keep their pixels bit for bit and get the status their input decides, and that nothing is NaN.  m_edge is reported and does
not gate (a sample within 1e-3 px of a validity edge occurred in most cases and moved no result measurably).

Measured, oracle against ref64 (printed by test_oracle_matches_ref64).  The cases: 31 full problems (28 comparable, the 3 of DEGENERATE),
the 24 one-step forms of the comparable ones that iterate more than once, and 16 batch problems; all 68 comparable, none skipped:
                   worst pixel   worst induced pixel   worst |dp|   worst |dq|   cond of H (2-norm)
  full             1.0e-4 px     4.3e-5 px             5.3e-7       7.7e-8       1.8e3 .. 4.6e3
  one step         7.7e-5 px     6.4e-4 px             1.9e-5       1.6e-6       1.7e3 .. 4.8e3
  batch problems   1.6e-4 px     3.8e-5 px             5.9e-7       5.6e-8       1.7e3 .. 2.4e3
smallest m_converge 0.0020 (loose-convergence; 0.027 otherwise), smallest m_z 0.080 (near-scene, depth 0.1; 3.97 otherwise).  A
converged pose forgets the rounding of its earlier steps; one step from a start 2.5 px away carries the float32 rounding of its
25 000 to 50 000-term sums (the oracle's wide-sum build, the same float32 products summed in double, agrees with ref64 to 2e-5 px
on the one-step cases where the float32 sums give 4.6e-4 to 6.4e-4 px).  The mutants are detected by factors of 143 to 1e5 or on a
decision.  The file runs in about 12 s.
"""
import functools

import numpy as np
import pytest

from feature_tracker_amd import synth
from tests import direct_ref64 as R64

TOL_PX = 1e-3     # per feature (north star), pixels and induced pixels
BAND_REL = 1e-3   # relative band round kMaxConvergeStep (the KLT check's)
BAND_Z = 1e-3     # band round kZeroFloat, in the unit of the points: a float32 pipeline's z at depth ~5 is good to ~1e-6
BAND_PX = 1e-3    # px from the outside bounds
TRUTH_PX = 0.5    # known answers: the px the existing translation test allows
DEGENERATE = {"textureless": "zero", "all-skipped": "zero", "single-feature": "rank"}

K640 = (400.0, 410.0, 321.5, 238.25)
K320 = (200.0, 205.0, 160.75, 119.125)
K333 = (300.0, 295.0, 165.5, 124.75)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def image_pair(w, h, shift=(3.3, -2.1), rotation_deg=0.0, scale=1.0):
    return synth.make_image_pair(w, h, shift, rotation_deg=rotation_deg, scale=scale)


def lift(uv, K, z):
    fx, fy, cx, cy = K
    return np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z * np.ones(len(uv))], axis=1).astype(np.float32)


def planar(w=640, h=480, levels=4, n=300, K=K640, seed=12345, half=6, rotation_deg=0.0, scale=1.0, depth=5.0, spread=True):
    """The scenes of tests/test_direct_method_gpu.py: a similarity-warped image pair, points at varied depths behind the features."""
    ref, cur = image_pair(w, h, (3.3, -2.1), rotation_deg, scale)
    uv = synth.make_features(n, w, h, seed=seed, half=half)
    rs = np.random.RandomState(seed)
    z = (depth * rs.uniform(0.8, 1.25, len(uv))).astype(np.float32) if spread else np.float32(depth)
    return synth.build_pyramid(ref, levels), synth.build_pyramid(cur, levels), uv, lift(uv, K, z)


def rotvec_quat(r):
    r = np.asarray(r, np.float64)
    a = np.linalg.norm(r)
    return np.array([1.0, 0, 0, 0]) if a == 0 else np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * r / a])


PLANE_N = np.array([0.15, -0.10, 1.0]) / np.linalg.norm([0.15, -0.10, 1.0])
PLANE_D = 5.0 * PLANE_N[2]  # the tilted plane n . X = d through (0, 0, 5)


@functools.lru_cache(maxsize=None)
def plane_view(w, h, K, q_rc, p_rc):
    """The second view of a textured, tilted plane from the pose (q_rc, p_rc) (X_ref = R_rc X_cur + p_rc).  The texture is
    synth.value_noise of the reference pixel.  Each current pixel is back-projected, its ray moved into the reference frame and
    cut with the plane, the cut projected into the reference image and the texture sampled there."""
    fx, fy, cx, cy = K
    vs, us = np.mgrid[0:h, 0:w].astype(np.float64)
    ref = np.floor(synth.value_noise(us, vs) + 0.5).astype(np.uint8)
    rays = np.stack([(us.ravel() - cx) / fx, (vs.ravel() - cy) / fy, np.ones(us.size)], 1) @ R64.q_matrix(np.array(q_rc)).T
    o = np.array(p_rc)
    t = (PLANE_D - PLANE_N @ o) / (rays @ PLANE_N)
    X = o + t[:, None] * rays
    cur = np.floor(synth.value_noise(fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy) + 0.5).astype(np.uint8).reshape(h, w)
    return np.ascontiguousarray(ref), np.ascontiguousarray(cur)


def plane_points(uv, K):
    fx, fy, cx, cy = K
    rays = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(len(uv))], 1).astype(np.float64)
    return (rays * (PLANE_D / (rays @ PLANE_N))[:, None]).astype(np.float32)


POSES = {  # true (rotation vector, translation) of the current camera in the reference frame
    "rot-x": ((0.010, 0.0, 0.0), (0.0, 0.0, 0.0)),
    "rot-y": ((0.0, -0.012, 0.0), (0.0, 0.0, 0.0)),
    "trans-z": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.20)),
    "general": ((0.006, -0.005, 0.035), (0.06, -0.04, 0.12)),
}
ROTATED = (0.03, -0.02, 0.0)
NEARBY = ((0.002, 0.0015, -0.003), (0.012, -0.008, 0.02))  # added to the truth for the nearby start


def case(name, rl, cl, K, pts, uv, cur=None, q=(1, 0, 0, 0), p=(0, 0, 0), status=None, truth=None, world=None, **opt):
    return dict(name=name, rl=list(rl), cl=list(cl), K=K, pts=pts, uv=uv, cur=cur, q=np.float32(q), p=np.float32(p), status=status, truth=truth,
                world=world, opt=opt)


def one_step(c):
    """The case on its finest level alone with kMaxIteration 1: a wrong Jacobian cannot hide behind convergence to the same fixed point."""
    d = dict(c, name=c["name"] + "/one-step", rl=c["rl"][:1], cl=c["cl"][:1], opt=dict(c["opt"], max_iteration=1), truth=None)
    return d


@functools.lru_cache(maxsize=None)
def full_cases():
    out = []
    rl, cl, uv, pts = planar(spread=False, seed=4321)
    out.append(case("translation-plane", rl, cl, K640, pts, uv, max_points=300, truth="translation"))
    for levels, half, n in [(1, 6, 120), (3, 4, 77), (5, 6, 300), (4, 2, 500), (2, 8, 33)]:
        rl, cl, uv, pts = planar(levels=levels, n=n, half=half, rotation_deg=0.4, scale=1.004)
        out.append(case(f"similarity/L{levels}-h{half}-n{n}", rl, cl, K640, pts, uv, half=half, max_points=n))
    # rectangular patches, half 0, an odd-sized image whose truncating pyramid drops a row or column at every level
    rl, cl, uv, pts = planar(levels=3, n=200, rotation_deg=0.4, scale=1.004)
    out.append(case("rect-3x7", rl, cl, K640, pts, uv, half=3, half_cols=7, max_points=200))
    out.append(case("rect-7x2", rl, cl, K640, pts, uv, half=7, half_cols=2, max_points=200))
    out.append(case("half-0", rl, cl, K640, pts, uv[:200], half=0, max_points=200))
    # a scene ten centimetres away: translation steps are small numbers beside the rotation steps, so the rotation part of |dx|^2
    # decides a convergence test
    rl, cl, uv, pts = planar(levels=2, n=200, rotation_deg=0.4, scale=1.004, depth=0.1)
    out.append(case("near-scene", rl, cl, K640, pts, uv, half=5, max_points=200))
    rl, cl, uv, pts = planar(333, 251, 3, 180, K333, half=5, rotation_deg=0.3, scale=1.003, seed=7)
    out.append(case("odd-333x251", rl, cl, K333, pts, uv, half=5, max_points=180))
    # a prediction, a start pose that is not the identity (nor of unit length), an incoming status vector and a cap below n
    rl, cl, uv, pts = planar(n=260)
    pred = (uv + np.float32([1.0, -0.5])).astype(np.float32)
    out.append(case("prediction+pose+status+cap", rl, cl, K640, pts, uv, pred, [0.9999, 0.003, -0.004, 0.002], [-0.02, 0.01, 0.005],
                    (np.arange(260) % 5).astype(np.uint8), max_points=200))
    # points behind the camera or below kZeroFloat stay at their prediction, some of it outside the image or exactly on its bounds
    rl, cl, uv, pts = planar(n=200)
    uv, pts = uv.copy(), pts.copy()
    pts[::7, 2] = -1.0
    pts[3::11, 2] = 5e-7
    pts[5::13, 2] = 0.0
    pred = uv.copy()
    pred[20:28] = np.float32([[-5.0, 10.0], [700.0, 10.0], [10.0, -3.0], [10.0, 500.0], [639.5, 100.0], [639.0, 100.0], [0.0, 50.0], [17.0, 479.0]])
    pts[20:28, 2] = -2.0
    out.append(case("skipped-points", rl, cl, K640, pts, uv, pred, max_points=200))
    rl, cl, uv, pts = planar(n=50)
    out.append(case("max-iteration-1/4-levels", rl, cl, K640, pts, uv, max_iteration=1))
    out.append(case("loose-convergence", rl, cl, K640, pts, uv, converge=1e-4, half=3))
    for method in ("inverse", "fast"):  # empty stubs: nothing moves, statuses are still produced
        out.append(case(f"stub-{method}", rl, cl, K640, pts, uv, uv + np.float32([300.0, 0.0]), method=method))
    # 3-D scenes: a tilted plane seen from a known pose, from the identity and from a nearby start
    uv = synth.make_features(150, 320, 240, seed=21, margin=30.0, half=4)
    pts = plane_points(uv, K320)
    for name, (rv, t) in POSES.items():
        q_true, p_true = rotvec_quat(rv), np.array(t, np.float64)
        ref, cur = plane_view(320, 240, K320, tuple(q_true), tuple(p_true))
        rl, cl = synth.build_pyramid(ref, 3), synth.build_pyramid(cur, 3)
        truth = (q_true, p_true)
        out.append(case(f"plane-{name}/identity-start", rl, cl, K320, pts, uv, half=4, max_points=150, truth=truth))
        q0 = rotvec_quat(np.add(rv, NEARBY[0]))
        out.append(case(f"plane-{name}/nearby-start", rl, cl, K320, pts, uv, None, q0, np.add(t, NEARBY[1]), half=4, max_points=150, truth=truth))
        if name == "general":  # a start whose rotation is large and 6 px away about x and y: dq and q_rc do not commute
            q0 = rotvec_quat(np.add(rv, ROTATED))
            out.append(case(f"plane-{name}/rotated-start", rl, cl, K320, pts, uv, None, q0, t, half=4, max_points=150, truth=truth))
    # the world-frame overload
    rl, cl, uv, pts = planar(n=150)
    ref_q = np.float32([0.98, 0.05, -0.12, 0.1])
    ref_q /= np.linalg.norm(ref_q)
    ref_p = np.float32([1.0, -2.0, 0.5])
    p_w = (R64.q_rotate(ref_q.astype(np.float64), pts.astype(np.float64)) + ref_p).astype(np.float32)
    out.append(case("world-frame", rl, cl, K640, p_w, uv, None, ref_q, ref_p, world=(ref_q, ref_p), max_points=150))
    # more tracked features than a workgroup's LDS table holds (768): the device keeps the per-feature table in device memory
    rl, cl, uv, pts = planar(levels=2, n=3500, half=1, rotation_deg=0.2, scale=1.002)
    out.append(case("many-features", rl, cl, K640, pts, uv, half=1, max_points=3500, max_iteration=6))
    # degenerate on purpose (DEGENERATE)
    flat = [np.full((240 >> k, 320 >> k), 90, np.uint8) for k in range(3)]
    fuv = np.float32([[100.5, 80.25], [200.0, 120.0], [30.0, 200.0]])
    out.append(case("textureless", flat, flat, K640, lift(fuv, K640, np.float32(4.0)), fuv))
    rl, cl, uv, pts = planar(n=40)
    behind = pts.copy()
    behind[:, 2] = -np.abs(behind[:, 2])
    out.append(case("all-skipped", rl, cl, K640, behind, uv, uv + np.float32([2.0, 1.0]), rotvec_quat((0.02, 0.0, -0.02)), [0.1, 0.0, -0.1]))
    out.append(case("single-feature", rl, cl, K640, pts[:3], uv[:3], uv[:3] + np.float32([1.5, -0.5]), max_points=1))
    return out


def is_one_step_source(c):
    return c["name"] not in DEGENERATE and not c["name"].startswith(("stub-", "max-iteration-1", "loose-"))


@functools.lru_cache(maxsize=None)
def one_step_cases():
    return [one_step(c) for c in full_cases() if is_one_step_source(c)]


@functools.lru_cache(maxsize=None)
def batch_cases():
    """Problems of different sizes for one device batch per pyramid depth (a batch shares its depth: the API refuses a mixed one)."""
    out = {}
    for levels in (1, 2, 4, 5):
        rl, cl, uv, pts = planar(levels=levels, n=300, rotation_deg=0.4, scale=1.004)
        out[levels] = [case(f"batch/L{levels}-n{n}", rl, cl, K640, np.ascontiguousarray(pts[k:k + n]), np.ascontiguousarray(uv[k:k + n]), max_points=500)
                       for k, n in enumerate((300 - 3, 150, 33, 77))]
    return out


def all_cases():
    return full_cases() + one_step_cases() + [c for cs in batch_cases().values() for c in cs]


def degenerate_kind(c):
    return DEGENERATE.get(c["name"].split("/")[0])


# ---- running a case ---------------------------------------------------------------------------------------------------------------

_REF = {}


def run_ref(c, flags=R64.DEFAULT):
    """ref64 on a case (the unmutated result is kept: the GPU file compares every launch form with it)."""
    if flags is R64.DEFAULT:
        if id(c) not in _REF:
            _REF[id(c)] = (c, _run_ref(c, flags))  # keyed on the case object (kept alive here), not on its name
        return _REF[id(c)][1]
    return _run_ref(c, flags)


def _run_ref(c, flags):
    if c["world"] is not None:
        rq, rp = c["world"]
        return R64.track_world(c["rl"], c["cl"], c["K"], rq, rp, c["pts"], c["uv"], c["cur"], c["q"], c["p"], c["status"], flags=flags, **c["opt"])
    return R64.track(c["rl"], c["cl"], c["K"], c["pts"], c["uv"], c["cur"], c["q"], c["p"], c["status"], flags=flags, **c["opt"])


def run_oracle(oracle, c):
    """(ok, uv, q, p, status, iterations).  The oracle has no world-frame entry: that overload is its exported quaternion algebra
    round its camera-frame entry, in float32, as tests/test_direct_method_gpu.py composes it."""
    if c["world"] is None:
        return oracle.direct_track(c["rl"], c["cl"], c["K"], c["pts"], c["uv"], c["cur"], c["q"], c["p"], c["status"], **c["opt"])
    rq, rp = c["world"]
    r_cw = oracle.quat_inverse(rq)
    p_c = np.stack([oracle.quat_rotate(r_cw, (pw - rp).astype(np.float32)) for pw in c["pts"]]).astype(np.float32)
    q0 = oracle.quat_mul(r_cw, c["q"])
    p0 = oracle.quat_rotate(r_cw, (c["p"] - rp).astype(np.float32))
    ok, uv, q, p, st, it = oracle.direct_track(c["rl"], c["cl"], c["K"], p_c, c["uv"], c["cur"], q0, p0, c["status"], **c["opt"])
    return ok, uv, oracle.quat_mul(rq, q), (oracle.quat_rotate(rq, p) + rp).astype(np.float32), st, it


def incoming_uv(c):
    n = len(c["uv"])
    given = c["cur"] is not None and len(c["cur"]) == n
    return np.asarray(c["cur"] if given else c["uv"], np.float32)


def camera_frame(c, q, p):
    """A pose of a world-frame case in the reference camera's frame (float64), for the induced pixels."""
    if c["world"] is None:
        return np.asarray(q, np.float64), np.asarray(p, np.float64)
    rq, rp = (np.asarray(a, np.float64) for a in c["world"])
    r_cw = R64.q_inverse(rq)
    return R64.q_mul(r_cw, np.asarray(q, np.float64)), R64.q_rotate(r_cw, np.asarray(p, np.float64) - rp)


def scene_depths(c):
    """The nearest and farthest depth of the points that are tracked: inside the cap and not below kZeroFloat in the reference
    frame.  (No such point in the all-skipped problem: there any range shows that nothing moved.)"""
    pts = np.asarray(c["pts"], np.float64)
    if c["world"] is not None:
        rq, rp = (np.asarray(a, np.float64) for a in c["world"])
        pts = R64.q_rotate(R64.q_inverse(rq), pts - rp)
    z = pts[:min(len(c["uv"]), c["opt"].get("max_points", 500)), 2]
    z = z[z >= R64.K_ZERO]
    return (float(z.min()), float(z.max())) if len(z) else (1.0, 5.0)


def induced_difference(c, qa, pa, qb, pb):
    rows, cols = c["rl"][0].shape
    G = R64.grid_points(c["K"], rows, cols, scene_depths(c))
    a, _ = R64.project(c["K"], *camera_frame(c, qa, pa), G)
    b, _ = R64.project(c["K"], *camera_frame(c, qb, pb), G)
    return float(np.abs(a - b).max())


def comparable(c, ref):
    """By ref64's own report (module docstring).  Returns a list of reasons why not (empty: comparable)."""
    why = []
    if ref.singular:
        why.append("singular")
    if not ref.m_converge > BAND_REL:
        why.append(f"m_converge {ref.m_converge:.3g}")
    if not ref.m_z > BAND_Z:
        why.append(f"m_z {ref.m_z:.3g}")
    if ref.ok and not (ref.m_outside >= BAND_PX).all():
        why.append(f"m_outside {ref.m_outside.min():.3g}")
    return why


def check(c, ref, got):
    """got = (ok, uv, q, p, status, iterations) of the implementation under test.  Returns (ok, message, failure factor, stats);
    a wrong decision (ok, a status, the iteration count, an unwritten pixel that moved) has the factor inf: its allowance is zero."""
    ok_g, uv_g, q_g, p_g, st_g, it_g = got
    uv_g = np.asarray(uv_g, np.float32)
    kind = degenerate_kind(c)
    bad, decision = [], False  # decision: a failure whose allowance is zero
    if bool(ok_g) != ref.ok:
        bad.append(f"ok {ok_g} vs {ref.ok}")
        decision = True
    stats = dict(px=0.0, induced=0.0, dp=0.0, dq=0.0, cond=ref.cond, m_converge=ref.m_converge, m_z=ref.m_z, m_edge=ref.m_edge,
                 iterations=ref.iters, capped=ref.capped)
    unwritten = ~ref.written
    if len(uv_g) != len(ref.uv) or len(st_g) != len(ref.status):
        return False, f"{c['name']}: sizes differ", np.inf, stats
    if not np.array_equal(uv_g[unwritten].view(np.uint32), incoming_uv(c)[unwritten].view(np.uint32)):
        bad.append("a pixel ref64 never wrote has moved")
        decision = True
    if kind == "rank":  # what is decided without the solver: the features beyond the cap, and that nothing is NaN
        if not np.array_equal(np.asarray(st_g, np.uint8)[unwritten], ref.status[unwritten]):
            bad.append("status of a feature beyond the cap")
        if not (np.isfinite(uv_g).all() and np.isfinite(q_g).all() and np.isfinite(p_g).all()):
            bad.append("not finite")
        return not bad, f"{c['name']}: {bad}", np.inf if bad else 0.0, stats
    if not np.array_equal(np.asarray(st_g, np.uint8), ref.status):
        bad.append(f"status differs at {np.nonzero(np.asarray(st_g) != ref.status)[0][:8]}")
        decision = True
    # H = 0 solves to dx = 0 under any rule, so the count of such a case is decided even though ref64 calls it singular
    if kind == "zero" or not (ref.capped or ref.m_converge <= BAND_REL):
        if int(it_g) != ref.iters:
            bad.append(f"iterations {it_g} vs {ref.iters}")
            decision = True
    w = ref.written
    stats["px"] = float(np.abs(uv_g[w].astype(np.float64) - ref.uv[w]).max()) if w.any() else 0.0
    stats["induced"] = induced_difference(c, ref.q, ref.p, q_g, p_g)
    stats["dp"] = float(np.abs(np.asarray(p_g, np.float64) - ref.p).max())
    stats["dq"] = float(np.abs(np.asarray(q_g, np.float64) - ref.q).max())
    factor = max(stats["px"], stats["induced"]) / TOL_PX
    if not factor <= 1.0:
        bad.append(f"px {stats['px']:.3g}, induced px {stats['induced']:.3g} (bar {TOL_PX})")
    return not bad, f"{c['name']}: {bad or 'ok'} {stats}", np.inf if decision else factor, stats


def aggregate(agg, stats):
    for k in ("px", "induced", "dp", "dq", "cond"):
        agg[k] = max(agg.get(k, 0.0), stats[k])
    for k in ("m_converge", "m_z", "m_edge"):
        agg[k] = min(agg.get(k, np.inf), stats[k])
    agg["cond_min"] = min(agg.get("cond_min", np.inf), stats["cond"] if stats["cond"] > 0 else np.inf)
    agg["cases"] = agg.get("cases", 0) + 1
    return agg


def check_all(run_impl, cases=None):
    """Every case through `run_impl(case)` -> (ok, uv, q, p, status, iterations); asserts the criterion, that every case outside
    DEGENERATE is comparable (none skipped), and returns the aggregate figures."""
    agg, skipped = {}, []
    for c in (all_cases() if cases is None else cases):
        ref = run_ref(c)
        if degenerate_kind(c) is None:
            why = comparable(c, ref)
            if why:
                skipped.append((c["name"], why))
                continue
        ok, msg, _, stats = check(c, ref, run_impl(c))
        assert ok, msg
        if degenerate_kind(c) is None:
            aggregate(agg, stats)
    assert not skipped, f"cases that ref64 reports as not comparable (give them another seed): {skipped}"
    return agg


# ---- 1. the oracle against ref64, every case -----------------------------------------------------------------------------------------

def test_there_are_enough_cases_and_every_one_is_comparable():
    assert len(full_cases()) >= 20 and len(one_step_cases()) >= 20
    names = [c["name"] for c in all_cases()]
    assert len(set(names)) == len(names)
    skipped = [(c["name"], comparable(c, run_ref(c))) for c in all_cases() if degenerate_kind(c) is None and comparable(c, run_ref(c))]
    assert len(skipped) == 0, skipped
    for c in all_cases():
        if degenerate_kind(c) is not None:  # degenerate by ref64's own report, not by name alone
            r = run_ref(c)
            assert r.singular and r.cond == 0.0, c["name"]
            if degenerate_kind(c) == "rank":
                assert r.written.tolist() == [True, False, False] and np.linalg.matrix_rank(_first_H(c)) <= 2
            if degenerate_kind(c) == "zero":  # nothing moved: the start pose (normalised), every level converged at once
                q0 = c["q"].astype(np.float64)
                assert np.abs(r.q - q0 / np.linalg.norm(q0)).max() < 1e-15 and np.array_equal(r.p, c["p"].astype(np.float64))
                assert r.iters == len(c["rl"]) and np.abs(r.uv[r.written] - incoming_uv(c)[r.written]).max(initial=0.0) < 1e-4


def _first_H(c):
    L = len(c["rl"])
    o = R64.Options(kMaxTrackPointsNumber=c["opt"].get("max_points", 500))
    H, _, _ = R64.normal_equations(R64._Image(c["rl"][-1]), R64._Image(c["cl"][-1]), np.float64(c["K"]) / 2 ** (L - 1), c["pts"],
                                   c["uv"] / np.float32(2 ** (L - 1)), incoming_uv(c).astype(np.float64), c["q"].astype(np.float64),
                                   c["p"].astype(np.float64), o, R64.DEFAULT)
    return H


def test_oracle_matches_ref64(oracle):
    for kind, cases in (("full", full_cases()), ("one-step", one_step_cases()), ("batch problems", [c for cs in batch_cases().values() for c in cs])):
        agg = check_all(lambda c: run_oracle(oracle, c), cases)
        print(f"\nDIRECT oracle vs ref64, {kind}: {agg}")


def test_the_cases_reach_the_launch_forms_they_are_meant_for():
    """ftk::direct_plan (a pure function, tests/test_match_plan_cpu.py) on the cases' sizes under the switches of the GPU file's forms:
    which cases the spread kernel takes, and that many-features keeps its table in device memory in every form."""
    from tests.test_match_plan_cpu import plan
    cases = [c for c in full_cases() + one_step_cases() if degenerate_kind(c) is None and c["opt"].get("method", "direct") == "direct"]
    forms = {"default": {}, "one-workgroup": dict(spread=0), "spread-3-tiny": dict(spread=3, min_terms=1), "tree": dict(tree=1)}
    for form, ov in forms.items():
        inputs = [dict(n_problems=1, max_features=min(len(c["uv"]), c["opt"].get("max_points", 500)), patch_rows=2 * c["opt"].get("half", 6) + 1,
                       patch_cols=2 * c["opt"].get("half_cols", c["opt"].get("half", 6)) + 1, **ov) for c in cases]
        plans = plan("direct", inputs)
        for c, i, pl in zip(cases, inputs, plans):
            in_lds = i["max_features"] <= 768
            assert pl["feat_in_global"] == int(not in_lds), (form, c["name"])
            if form == "default":
                assert pl["producers"] == (32 if in_lds and i["max_features"] * i["patch_rows"] * i["patch_cols"] >= 64 * 256 else 0), (form, c["name"])
            elif form == "spread-3-tiny":
                assert pl["producers"] == (3 if in_lds else 0), (form, c["name"])
            else:
                assert pl["producers"] == 0, (form, c["name"])
        spread = sum(1 for pl in plans if pl["producers"] > 0)
        print(f"\nLAUNCH FORMS {form}: {spread} of {len(cases)} cases spread, {sum(pl['feat_in_global'] for pl in plans)} with the table in device memory")
        if form == "default":
            assert spread >= 15 and len(cases) - spread >= 15
        assert sum(pl["feat_in_global"] for pl in plans) == 2  # many-features, full and one-step
    batch = plan("direct", [dict(n_problems=4, max_features=297, patch_rows=13, patch_cols=13)])[0]
    assert batch["producers"] == 32 and batch["grid"] == (4 * 33, 1)  # the device batches of the GPU file: each problem spread


# ---- 2. known answers ----------------------------------------------------------------------------------------------------------------

def _implementations(oracle):
    return {"ref64": lambda c: (lambda r: (r.ok, r.uv, r.q, r.p, r.status, r.iters))(run_ref(c)), "oracle": lambda c: run_oracle(oracle, c)}


def test_true_pose_is_recovered_on_the_3d_scenes(oracle):
    """The pixels the recovered pose induces on the scene's points against those of the true pose, within TRUTH_PX."""
    for who, run in _implementations(oracle).items():
        n = 0
        for c in full_cases():
            if c["truth"] is None:
                continue
            ok, uv, q, p, st, it = run(c)
            if c["truth"] == "translation":  # a fronto-parallel plane at depth 5 whose image moves by (+3.3, -2.1) px
                q_true, p_true = np.array([1.0, 0, 0, 0]), np.array([-3.3 * 5.0 / K640[0], 2.1 * 5.0 / K640[1], 0.0])
            else:
                q_true, p_true = c["truth"]
            want, _ = R64.project(c["K"], q_true, p_true, c["pts"])
            have, _ = R64.project(c["K"], q, p, c["pts"])
            d = np.abs(want - have).max()
            print(f"\nTRUTH {who} {c['name']}: {d:.3g} px, {it} iterations")
            assert ok and d <= TRUTH_PX, (who, c["name"], d)
            assert np.abs(np.asarray(uv, np.float64) - want).max() <= TRUTH_PX, (who, c["name"])
            n += 1
        assert n == 10


def _ramp(shift, w=128, h=64):
    x = np.arange(w, dtype=np.int32)
    return np.tile((2 * x).clip(0, 255).astype(np.uint8), (h, 1)), np.tile((2 * (x - shift)).clip(0, 255).astype(np.uint8), (h, 1))


def test_hand_derived_step_on_the_ramp_I_equals_2x(oracle):
    """ref = 2x, cur = 2(x - 1): the scene moved by +1 px in x.  One feature at the principal point, depth Z, identity start: the
    point projects onto its own reference pixel, so every patch pixel has gx = (2(x+1) - 2(x-1)) / 2 = 2, gy = 0 and the residual
    cur - ref = -2.  With X = Y = 0 the Jacobian's first row is (fx/Z, 0, 0, 0, fx, 0), so every term is jac = 2 (fx/Z, 0, 0, 0, fx, 0):
    over the P = 25 patch pixels H[0][0] = 4 P fx^2 / Z^2, b[0] = -4 P fx / Z, and the translation that solves H dx = b alone is
    dx[0] = b[0] / H[0][0] = -Z / fx: the camera moves one pixel's worth to the left, the image one pixel to the right.
    H = P jac jac^T has rank 1, so dx is fixed only along jac: every solution has jac . dx = -2, i.e. moves the point's pixel by
    +1 px to first order (the second-order term of the rotation part is (1/fx)^2 fx / 2 < 2e-3 px)."""
    ref, cur = _ramp(1)
    fx, fy, cx, cy, Z = 300.0, 300.0, 60.0, 30.0, 2.0
    K = (fx, fy, cx, cy)
    uv, pts = np.float32([[cx, cy]]), np.float32([[0.0, 0.0, Z]])
    o = R64.Options(kPatchRowHalfSize=2, kPatchColHalfSize=2)
    H, b, ids = R64.normal_equations(R64._Image(ref), R64._Image(cur), np.float64(K), pts, uv, uv.astype(np.float64), np.array([1.0, 0, 0, 0]),
                                     np.zeros(3), o, R64.DEFAULT)
    assert H[0, 0] == 4 * 25 * fx * fx / (Z * Z) and b[0] == -4 * 25 * fx / Z and ids.tolist() == [0]
    hand = np.array([-Z / fx, 0, 0, 0, 0, 0])
    assert np.abs(H @ hand - b).max() <= 1e-9 * np.abs(b).max()
    c = case("ramp", [ref], [cur], K, pts, uv, half=2, max_iteration=1)
    for who, run in _implementations(oracle).items():
        ok, _, q, p, st, it = run(c)
        px, _ = R64.project(K, q, p, pts)
        assert ok and it == 1 and abs(px[0, 0] - (cx + 1.0)) < 5e-3 and abs(px[0, 1] - cy) < 5e-3, (who, px)
    assert run_ref(c).singular


def test_stubs_move_nothing_and_still_produce_statuses(oracle):
    for who, run in _implementations(oracle).items():
        for c in full_cases():
            if not c["name"].startswith("stub-"):
                continue
            ok, uv, q, p, st, it = run(c)
            assert ok and it == 0 and np.array_equal(np.asarray(uv, np.float32), c["cur"]), who
            assert np.array_equal(np.asarray(q, np.float32), c["q"]) and np.array_equal(np.asarray(p, np.float32), c["p"])
            want = np.where(c["cur"][:, 0] > 639.0, R64.OUTSIDE, R64.TRACKED)
            assert np.array_equal(st, want) and (want == R64.OUTSIDE).any() and (want == R64.TRACKED).any(), who


def test_world_frame_overload_is_the_camera_frame_overload_composed_by_hand():
    c = next(c for c in full_cases() if c["name"] == "world-frame")
    rq, rp = (np.asarray(a, np.float64) for a in c["world"])
    w = run_ref(c)
    Rw = R64.q_matrix(rq)
    p_c = (c["pts"].astype(np.float64) - rp) @ Rw  # R^T (X - t), row vectors
    r = R64.track(c["rl"], c["cl"], c["K"], p_c, c["uv"], **c["opt"])  # the start pose is the reference's: identity in its frame
    assert r.ok and w.ok and r.iters == w.iters and np.array_equal(r.status, w.status)
    assert np.abs(r.uv - w.uv).max() < 1e-4  # the lifted points round to float32 from two float64 values that differ in their last bits
    assert np.abs(Rw @ r.p + rp - w.p).max() < 1e-6 and np.abs(Rw @ R64.q_matrix(r.q) - R64.q_matrix(w.q)).max() < 1e-6


def test_refusals_cap_prediction_rule_and_status_pass(oracle):
    rl, cl, uv, pts = planar(levels=2, n=40)
    cur3 = synth.build_pyramid(cl[0], 3)
    for who, run in _implementations(oracle).items():
        assert run(case("mismatch", rl, cur3, K640, pts, uv))[0] is False, who  # :39
        assert run(case("empty", rl, cl, K640, pts[:0], uv[:0]))[0] is False, who  # :38
        # sizes differ: no prediction (:42-44); a status vector of another size is reset to kTracked (:74-76)
        a = run(case("a", rl, cl, K640, pts, uv, uv[:7] + np.float32([3.0, 3.0]), status=np.full(9, 2, np.uint8)))
        b = run(case("b", rl, cl, K640, pts, uv))
        assert a[0] and np.array_equal(np.asarray(a[1]), np.asarray(b[1])) and (np.asarray(a[4]) == R64.TRACKED).all(), who
        # the cap: features beyond it are neither used nor moved; a valid status vector is kept
        pred = uv + np.float32([1.5, -0.5])
        st = (np.arange(40) % 5).astype(np.uint8)
        d = run(case("d", rl, cl, K640, pts, uv, pred, status=st, max_points=25))
        assert np.array_equal(np.asarray(d[1], np.float32)[25:], pred[25:]) and np.array_equal(np.asarray(d[4]), st), who
        e = run(case("e", rl, cl, K640, pts[:25], uv[:25], pred[:25]))
        assert np.abs(np.asarray(d[2], np.float64) - e[2]).max() == 0 and np.abs(np.asarray(d[3], np.float64) - e[3]).max() == 0, who
    r = R64.track(rl, cl, K640, pts, uv, max_points=25)
    assert r.written[:25].all() and not r.written[25:].any() and np.isinf(r.m_outside[25:]).all()


def test_cur_pixel_uv_lags_the_returned_pose_by_one_update():
    """The two facts of the source a test has to handle (direct_ref64's docstring)."""
    c = next(c for c in one_step_cases() if c["name"].startswith("plane-general/nearby"))
    r = run_ref(c)
    start, _ = R64.project(c["K"], c["q"].astype(np.float64), c["p"].astype(np.float64), c["pts"])
    end, _ = R64.project(c["K"], r.q, r.p, c["pts"])
    assert np.abs(r.uv - start).max() < 1e-9 and np.abs(r.uv - end).max() > 0.05
    s = run_ref(next(c for c in full_cases() if c["name"] == "skipped-points"))
    assert (~s.written).sum() > 40 and (s.status[20:24] == R64.OUTSIDE).all() and (s.status[24] == R64.OUTSIDE) and (s.status[25:28] == R64.TRACKED).all()


# ---- 3. the check can fail: mutants of ref64 -----------------------------------------------------------------------------------------

MUTANTS = {
    "gradient_without_half": (R64.Flags(no_half_gradient=True), "one"),
    "jacobian_at_current_point": (R64.Flags(jacobian_at_current_point=True), "one"),
    "rotation_column_sign": (R64.Flags(flip_rotation_column=4), "one"),
    "columns_3_4_swapped": (R64.Flags(swap_columns_3_4=True), "one"),
    "update_on_the_right": (R64.Flags(update_on_the_right=True), "one"),
    "no_inverse_in_projection": (R64.Flags(no_inverse=True), "one"),
    "principal_point_not_scaled": (R64.Flags(principal_point_not_scaled=True), "full"),
    "uv_from_updated_pose": (R64.Flags(uv_from_updated_pose=True), "one"),
    "bilinear_fractions_swapped": (R64.Flags(swap_sr_sc=True), "one"),
    "converge_on_translation_only": (R64.Flags(converge_on_translation_only=True), "full"),
    "outside_inclusive": (R64.Flags(outside_inclusive=True), "one"),
}


def mutant_factor(oracle, flags, kind):
    """The largest failure factor of the criterion over the cases of `kind`, the mutant in ref64's place (stops once past 1e3)."""
    worst, where = 0.0, None
    for c in (one_step_cases() if kind == "one" else full_cases()):
        if degenerate_kind(c) is not None:
            continue
        ok, _, f, _ = check(c, run_ref(c, flags), run_oracle(oracle, c))
        if not ok and f > worst:
            worst, where = f, c["name"]
        if worst >= 1e3:
            break
    return worst, where


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_of_ref64_is_detected(oracle, name):
    flags, kind = MUTANTS[name]
    factor, where = mutant_factor(oracle, flags, kind)
    print(f"\nMUTANT {name} ({kind}): detected with factor {factor:.3g} on {where}")
    assert factor >= 10.0, (name, factor)
