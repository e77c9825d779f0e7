"""The restatement of PnpRansac's "p3p" sampler (tests/pnp_p3p_ref.c) pinned without a device: the solver alone against
the properties of any P3P solver and against an independent float64 statement (tests/pnp_p3p_ref64.py: another quartic, numpy.roots,
Kabsch), the whole call against that statement and against ground truth on the 24-pose family, the separation of gross outliers, the
planar cases that the six-point DLT cannot solve, degenerate samples, and the mutants that these checks must catch.
tests/test_pnp_p3p_gpu.py then holds the kernel to the restatement bit for bit."""
import functools

import numpy as np
import pytest

from tests import epipolar_ref as E
from tests import pnp_p3p_ref as Q
from tests import pnp_p3p_ref64 as Q64
from tests import pnp_ref as R
from tests.test_pnp_cpu import MARGIN_MULTIPLE, MIN_DEPTH, NOISES, _angle, _invalid, _pose64, _status, _truth_errors

# The solver alone on noise-free samples whose quartic (float64) has its roots at least ROOT_GAP apart: the least the float32 quartic can
# be asked to tell apart (closer roots merge or part under the rounding of its coefficients, and the count and the poses go with them).
ROOT_GAP = 0.02
SAMPLES_PER_SCENE = 12
# 4 x the worst deviation measured on those samples: |R^T R - I| and |det R - 1|, the calibrated reprojection of the three
# sample points, the entries of [R | t] against the nearest float64 solution, and the true pose against the nearest returned solution
MEASURED_SOLVER = dict(orthonormal=3.21e-3, reprojection=8.55e-7, float64=1.60e-2, truth=3.58e-3)
SOLVER_TOLERANCE = {k: 4 * v for k, v in MEASURED_SOLVER.items()}
# the whole call against the float64 statement (radians, scene units), and against ground truth per noise: 4 x measured
MEASURED = (5.25e-5, 2.31e-4)  # (at 0.3 px and 0.5 px threshold the two statements may crown different hypotheses: rows at the threshold differ)
MEASURED_TRUTH = {0.0: (1.70e-7, 8.97e-7), 0.3: (8.42e-4, 5.31e-3)}
ROTATION_TOLERANCE, POSITION_TOLERANCE = (4 * v for v in MEASURED)
TRUTH_TOLERANCE = {noise: tuple(4 * v for v in m) for noise, m in MEASURED_TRUTH.items()}
SOLUTION_COUNTS = {1, 2, 3, 4}  # what the solver returns somewhere on these inputs (0: a hypothesis whose roots all fail a test)


def _contract(variant=Q.CONTRACT):
    return functools.partial(Q.solve, variant=variant)


@functools.lru_cache(maxsize=None)
def solver_samples():
    """(xy [3, 2] float32, X [3, 3] float32, (R, t) or None when the pixels carry no exact pose, float64 solutions) drawn from the family, the
    coplanar scene and the wide view, kept where the float64 roots stand ROOT_GAP apart."""
    rng = np.random.default_rng(0)
    scenes = [R.family_scene(name, 300, 1)[:2] + (R.family_scene(name, 300, 1)[3], R.K) for name in R.FAMILY]
    Xc, uvc, _ = R.case("coplanar")
    scenes.append((Xc, uvc, Q.coplanar_truth(), R.K))
    Xw, uvw, _, truth = R.wide_case()
    scenes.append((Xw, uvw, truth, R.K_WIDE))
    out, drawn = [], 0
    for X, uv, truth, K in scenes:
        xy = Q.calibrated(uv, K)
        for _ in range(SAMPLES_PER_SCENE):
            idx = rng.choice(len(X), 3, replace=False)
            drawn += 1
            found = Q64.p3p(xy[idx], X[idx])
            if found is not None and found[1] >= ROOT_GAP:
                out.append((xy[idx], X[idx], truth, found[0]))
    assert len(out) >= drawn // 2, (len(out), drawn)
    return out


def check_solver(variant=Q.CONTRACT):
    worst, counts = dict.fromkeys(MEASURED_SOLVER, 0.0), set()
    for xy, X, (Rt, tt), want in solver_samples():
        n, sols = Q.solver(xy, X, variant)
        counts.add(n)
        assert n == len(want), (n, len(want))
        near_truth = np.inf
        for P in sols.astype(np.float64):
            Rm, t = P[:, :3], P[:, 3]
            c = X.astype(np.float64) @ Rm.T + t
            assert (c[:, 2] > 0).all()
            dev = dict(orthonormal=max(np.abs(Rm.T @ Rm - np.eye(3)).max(), abs(np.linalg.det(Rm) - 1.0)),
                       reprojection=np.abs(c[:, :2] / c[:, 2:] - xy).max(),
                       float64=min(max(np.abs(Rm - a).max(), np.abs(t - b).max()) for a, b in want))
            near_truth = min(near_truth, max(np.abs(Rm - Rt).max(), np.abs(t - tt).max()))
            for key, v in dev.items():
                worst[key] = max(worst[key], v)
                assert v <= SOLVER_TOLERANCE[key], (key, v)
        worst["truth"] = max(worst["truth"], near_truth)
        assert near_truth <= SOLVER_TOLERANCE["truth"], near_truth  # noise-free: the true pose is among the solutions
    return worst, counts


def check_float64(solve):
    """As tests/test_pnp_cpu.py's: the family with 30 % outliers, noise-free and at 0.3 px, threshold 0.5 px, and K_OTHER (fx != fy)."""
    worst = np.zeros(2)
    cases = [(name, noise, R.K) for name in R.FAMILY for noise in NOISES] + [(name, 0.3, R.K_OTHER) for name in R.SHEPPERD_POSES]
    for name, noise, K in cases:
        X, uv, _, _ = R.family_scene(name, 300, 1, noise, 0.3, K)
        r, r64 = solve(X, uv, _status(300), K=K, threshold=0.5), Q64.solve(X, uv, _status(300), K, threshold=0.5)
        assert int(r.valid[0]) == 1 and r64.valid == 1, (name, noise)
        Rm, _, p = _pose64(r.pose)
        dev = np.array([_angle(Rm, r64.R), np.linalg.norm(p + r64.R.T @ r64.t)])
        worst = np.maximum(worst, dev)
        assert dev[0] <= ROTATION_TOLERANCE and dev[1] <= POSITION_TOLERANCE, (name, noise, dev)
        kept = r.status == R.TRACKED
        band = MARGIN_MULTIPLE * float(np.float32(K[0])) * (MEASURED[0] + MEASURED[1] / MIN_DEPTH)
        differ = np.flatnonzero(kept != r64.kept)
        assert (np.abs(r64.margin[differ]) <= band).all(), (name, noise, r64.margin[differ])
        assert int(r.n_inliers[0]) == int(kept.sum()) and (r.status[~kept] == R.LARGE_RESIDUAL).all()
    return worst


def check_ground_truth(solve):
    worst = {noise: np.zeros(2) for noise in NOISES}
    for name in R.FAMILY:
        for noise in NOISES:
            X, uv, _, truth = R.family_scene(name, 300, 1, noise, 0.3)
            r = solve(X, uv, _status(300))
            assert int(r.valid[0]) == 1
            err = _truth_errors(r.pose, truth)
            worst[noise] = np.maximum(worst[noise], err)
            assert (err <= TRUTH_TOLERANCE[noise]).all(), (name, noise, err)
    return worst


def check_separation(solve):
    """On all 24 poses at 300 points, 30 % gross outliers, 512 hypotheses and 1 px: no outlier is kept; noise-free every true inlier is."""
    for name in R.FAMILY:
        for noise in NOISES:
            X, uv, is_inlier, _ = R.family_scene(name, 300, 1, noise, 0.3)
            r = solve(X, uv, _status(300), hypotheses=512, threshold=1.0)
            kept = r.status == R.TRACKED
            assert not kept[~is_inlier].any(), (name, noise)
            if noise == 0.0:
                assert kept[is_inlier].all(), (name, int(kept.sum()))


def check_every_hypothesis_counts_its_sample(solve):
    """Noise-free and without outliers the fourth point finds the true pose among the solutions of most samples (an ill-conditioned
    sample's float32 pose may miss the 1 px of rows far from it, its own among them: no count is asked of every hypothesis)."""
    for name in R.SHEPPERD_POSES:
        X, uv, _, _ = R.family_scene(name, 300, 1)
        r = solve(X, uv, _status(300))
        assert (r.counts >= 0).sum() >= 400 and (r.counts == 300).sum() >= 300, name


K_ANISOTROPIC = (300.0, 900.0, 319.5, 239.5)
COUNTS_MAY_DIFFER = 4  # hypotheses of 512 whose count may differ from the float64 statement's by more than 2: 4 x the one measured


def check_unequal_focal_lengths_choose_by_pixels(solve):
    """fy = 3 fx at 0.3 px noise: the fourth point's error weighs its y part by fy / fx, as the float64 statement's does, so both choose the
    same solution and count the same rows, but for the hypotheses whose two best solutions lie within rounding of each other."""
    X, uv, _, _ = R.family_scene("small/side", 300, 1, 0.3, 0.3, K_ANISOTROPIC)
    r, r64 = solve(X, uv, _status(300), K=K_ANISOTROPIC), Q64.solve(X, uv, _status(300), K_ANISOTROPIC)
    differ = int((np.abs(r.counts - r64.counts) > 2).sum())
    assert differ <= COUNTS_MAY_DIFFER, differ
    return differ


def check_a_fourth_point_behind_the_camera(variant=Q.CONTRACT):
    """Three points of a scene and a fourth landmark that every float64 solution of the three puts behind the camera: no hypothesis."""
    X, uv, _, (Rt, tt) = R.family_scene("small/side", 300, 1)
    tried = 0
    for first in range(0, 296, 4):
        rows = list(range(first, first + 4))
        xy, X4 = Q.calibrated(uv[rows]), X[rows].copy()
        X4[3] = (Rt.T @ (np.array([0.1, -0.2, -40.0]) - tt)).astype(np.float32)  # 40 units behind the true camera
        found = Q64.p3p(xy[:3], X4[:3])
        if found is None or found[1] < ROOT_GAP or not all((Rm @ X4[3] + t)[2] < -1.0 for Rm, t in found[0]):
            continue
        tried += 1
        ok, P, n = Q.hypothesis(xy, X4, 1.0, variant)
        assert n >= 1 and not ok and not P.any(), rows
    assert tried >= 3, tried


def check_choice_at_a_tie(variant=Q.CONTRACT):
    """Among equal errors the solution produced first wins."""
    assert Q.choose([2.0, 1.0, 1.0, 3.0], variant) == 1 and Q.choose([1.0, 1.0], variant) == 0 and Q.choose([4.0, 3.0, 2.0], variant) == 2


CHECKS = {"fourth_point_ignored": lambda v: check_every_hypothesis_counts_its_sample(_contract(v)),
          "front_of_the_sample_not_tested": check_a_fourth_point_behind_the_camera,
          "tie_takes_the_last": lambda v: check_choice_at_a_tie(v),
          "y_error_unscaled": lambda v: check_unequal_focal_lengths_choose_by_pixels(_contract(v)),
          "one_newton_step_fewer": check_solver}  # (without the step a root misses the residual test: a solution is lost)


def check_behind(solve):
    """Every landmark behind the camera that sees it: no hypothesis may put its four points in front AND see more than its sample, and
    the result keeps next to nothing."""
    X, uv, status = R.case("behind")
    r = solve(X, uv, status)
    assert int(r.n_inliers[0]) <= BEHIND_KEPT, int(r.n_inliers[0])


BEHIND_KEPT = 8  # measured on the restatement: a twin pose of some triangle that a few more rows happen to agree with


@pytest.mark.parametrize("check", [check_float64, check_ground_truth, check_separation, check_every_hypothesis_counts_its_sample,
                                   check_unequal_focal_lengths_choose_by_pixels, check_behind], ids=lambda c: c.__name__)
def test_the_restatement_passes(check):
    check(_contract())


def test_the_solver_alone():
    worst, counts = check_solver()
    print("solver:", {k: f"{v:.3e}" for k, v in worst.items()}, "counts", sorted(counts))
    check_choice_at_a_tie()
    check_a_fourth_point_behind_the_camera()


@pytest.mark.parametrize("mutant", sorted(Q.MUTANTS))
def test_each_mutant_is_caught(mutant):
    with pytest.raises(AssertionError):
        CHECKS[mutant](Q.MUTANTS[mutant])


def test_the_tolerances_are_the_measured_deviations_with_their_margin():
    solver, _ = check_solver()
    worst, truth = check_float64(_contract()), check_ground_truth(_contract())
    print("solver:", {k: f"{v:.3e}" for k, v in solver.items()}, f"; against float64: rotation {worst[0]:.3e} rad, position {worst[1]:.3e}; against truth: " +
          "; ".join(f"noise {n}: rotation {truth[n][0]:.3e}, position {truth[n][1]:.3e}" for n in NOISES))
    pairs = [(SOLVER_TOLERANCE[k], solver[k]) for k in MEASURED_SOLVER] + list(zip((ROTATION_TOLERANCE, POSITION_TOLERANCE), worst))
    for noise in NOISES:
        pairs += list(zip(TRUTH_TOLERANCE[noise], truth[noise]))
    for tolerance, measured in pairs:
        assert tolerance / 8 <= measured <= tolerance  # no more than 8 x what is measured: it was not set loose


# ---- the planar cases ---------------------------------------------------------------------------------------------------------------------

def test_landmarks_of_one_plane_give_a_pose_under_p3p_and_none_under_dlt6():
    X, uv, status = R.case("coplanar")
    assert _invalid(R.solve(X, uv, status), status)
    r = Q.solve(X, uv, status)
    assert int(r.valid[0]) == 1 and int(r.n_inliers[0]) == 40 and (r.status == R.TRACKED).all()
    assert (_truth_errors(r.pose, Q.coplanar_truth()) <= TRUTH_TOLERANCE[0.0]).all()


def test_a_tilted_plane_with_outliers():
    X, uv, is_inlier, truth = Q.tilted_plane()
    assert np.abs(np.linalg.svd(X - X.mean(0), compute_uv=False)[-1]) <= 1e-4  # one plane
    assert int(R.solve(X, uv, _status(300)).n_inliers[0]) < int(is_inlier.sum())  # "dlt6": no pose of the plane
    r = Q.solve(X, uv, _status(300))
    assert int(r.valid[0]) == 1 and np.array_equal(r.status == R.TRACKED, is_inlier)
    assert (_truth_errors(r.pose, truth) <= TRUTH_TOLERANCE[0.0]).all()


# ---- degenerate samples and edges ---------------------------------------------------------------------------------------------------------

def _sample_of(name, rows=(0, 1, 2, 3)):
    X, uv, _ = Q.case(name)
    return Q.calibrated(uv[list(rows)]), X[list(rows)]


@pytest.mark.parametrize("name,rows", [("collinear", (0, 7, 21, 30)), ("coincident", (0, 1, 2, 5)), ("identical", (0, 1, 2, 3)), ("zeros", (0, 5, 6, 21)),
                                       ("hostile", (3, 5, 9, 14)), ("hostile", (0, 14, 1, 2)), ("hostile", (0, 1, 17, 23))])
def test_a_degenerate_sample_is_invalid(name, rows):
    xy, X = _sample_of(name, rows)
    with np.errstate(all="ignore"):
        ok, P, _ = Q.hypothesis(xy, X)
        n, _ = Q.solver(xy[:3], X[:3])
    assert not ok and not P.any() and n <= 0, (name, n)


def test_the_true_pose_of_a_sample_behind_the_camera_is_not_taken():
    """The sample's own (mirrored) pose has four negative depths: whatever is valid is another pose, with all four in front."""
    X, uv, _ = R.case("behind")
    for rows in ((0, 1, 2, 3), (4, 9, 17, 30), (5, 6, 7, 8)):
        ok, P, _ = Q.hypothesis(Q.calibrated(uv[list(rows)]), X[list(rows)])
        if ok:
            assert ((X[list(rows)].astype(np.float64) @ P[:, :3].T.astype(np.float64) + P[:, 3]) [:, 2] > 0).all()


@pytest.mark.parametrize("name", ["collinear", "identical"])
def test_degenerate_scenes_are_invalid(name):
    X, uv, status = Q.case(name)
    r = Q.solve(X, uv, status)
    assert _invalid(r, status) and (r.counts == -1).all() and not r.models.any() and (r.solutions == -1).all()


@pytest.mark.parametrize("name", ["zeros", "hostile", "coincident", "behind"])
def test_hostile_scenes_end_and_touch_no_row_that_takes_no_part(name):
    X, uv, status = Q.case(name)
    r = Q.solve(X, uv, status)
    part = np.isfinite(X).all(1) & np.isfinite(uv).all(1) & X.any(1)
    assert np.isfinite(r.pose).all() and np.isfinite(r.models).all() and (r.status[~part] == R.TRACKED).all()
    if name != "behind":
        assert int(r.valid[0]) == 1 and int(r.n_inliers[0]) >= 30


def test_few_participants():
    for m, valid in ((3, False), (4, True), (5, True), (6, True), (7, True)):
        X, uv, status = Q.case(f"n{m}")
        r = Q.solve(X, uv, status)
        if not valid:
            assert _invalid(r, status) and (r.counts == -1).all()
        else:
            assert int(r.valid[0]) == 1 and int(r.n_inliers[0]) == m
            # fewer than six rows end the refit at its first step: the pose is stage 4's
            assert (r.trace[R.TRACE_STEP0] == R.STEP_FEW_INLIERS and E.same(r.pose, Q.solve(X, uv, status, refine_iterations=0).pose)) == (m < Q.REFIT_MIN)


def test_the_trace_shows_every_solution_count():
    seen = set()
    for name in R.SHEPPERD_POSES:
        X, uv, _, _ = R.family_scene(name, 300, 1, 0.3, 0.3)
        seen |= set(np.unique(Q.solve(X, uv, _status(300)).solutions).tolist())
    X, uv, status = R.case("coplanar")
    seen |= set(np.unique(Q.solve(X, uv, status).solutions).tolist())
    assert seen == SOLUTION_COUNTS | {0}, seen


def test_two_calls_give_equal_bits_and_the_seed_matters():
    X, uv, _, _ = R.scene(300, 2, noise=0.3, outlier_share=0.3)
    a, b, c = (Q.solve(X, uv, _status(300), seed=s) for s in (4, 4, 5))
    assert R.same_results(a, b, R.OUTPUTS + R.HYPOTHESES) == [] and "models" in R.same_results(a, c, R.HYPOTHESES)
