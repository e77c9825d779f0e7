"""The restatement of PnpRansac (tests/pnp_ref.c) pinned without a device: against an independent float64 restatement
(tests/pnp_ref64.py: SVD null vectors, SVD rotation, numpy's solve), against ground truth on the 24-pose family of tests/two_view_pose_ref.py
at 300 points with and without 0.3 px noise, the separation of gross outliers as a condition, the summation tree restated apart in numpy,
the edge cases of the contract, and five mutants that the same checks must each catch.  tests/test_pnp_gpu.py then holds the kernels to
the restatement bit for bit."""
import functools

import numpy as np
import pytest

from tests import direct_ref64 as D64
from tests import epipolar_ref as E
from tests import pnp_ref as R
from tests import pnp_ref64 as R64
from tests import two_view_pose_ref as P
from tests import two_view_ref as T

NOISES = (0.0, 0.3)
# against the float64 restatement, 4 x the worst deviation measured over the family: radians between the two rotations,
# distance between the two camera positions (the scenes are about 6 units deep)
MEASURED = (2.02e-7, 1.94e-6)
ROTATION_TOLERANCE, POSITION_TOLERANCE = (4 * v for v in MEASURED)
# against ground truth, 4 x the worst error measured: noise-free, and at 0.3 px noise
MEASURED_TRUTH = {0.0: (2.09e-7, 1.22e-6), 0.3: (8.42e-4, 5.31e-3)}
TRUTH_TOLERANCE = {noise: tuple(4 * v for v in m) for noise, m in MEASURED_TRUTH.items()}
# the winner's pose before any refit step against ground truth, noise-free and without outliers, 4 x the worst error measured
MEASURED_STAGE4 = (8.70e-5, 1.24e-3)
STAGE4_TOLERANCE = tuple(4 * v for v in MEASURED_STAGE4)
# A row may differ from float64 in its final status only within this multiple of what the measured deviations move a projection by:
# fx (d_rotation + d_position / depth) pixels at the least depth of the scenes.
MARGIN_MULTIPLE = 2.0
MIN_DEPTH = 1.5
# the three restatements composed (two-view filter, TwoViewPose, PnpRansac) on a noise-free three-view sequence with 30 % outliers: view 2
# against ground truth up to the baseline's scale, 4 x the error measured
COMPOSED_POSES = ("small/side", "y130/back")
MEASURED_COMPOSED = (7.23e-4, 3.35e-3)
COMPOSED_ROTATION_TOLERANCE, COMPOSED_POSITION_TOLERANCE = (4 * v for v in MEASURED_COMPOSED)
# Outlier separation (a condition): every family pose is listed; one where the restatement itself missed would be left out here with the reason.
SEPARATION_POSES = R.FAMILY


def _contract(variant=R.CONTRACT):
    return functools.partial(R.solve, variant=variant)


def _status(n):
    return np.full(n, R.TRACKED, np.uint8)


def _angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0)))


def _pose64(pose):
    """(R, t, p_rc) with X_cur = R X + t of a pose [7], float64."""
    q = np.asarray(pose[:4], np.float64)
    Rrc = D64.q_matrix(q / np.linalg.norm(q))  # (a float32 quaternion is a unit one to 6e-8 only: arccos would turn that into 3e-4 rad)
    p = np.asarray(pose[4:], np.float64)
    return Rrc.T, -Rrc.T @ p, p


def _truth_errors(pose, truth):
    Rt, tt = truth
    Rm, _, p = _pose64(pose)
    return np.array([_angle(Rm, Rt), np.linalg.norm(p + Rt.T @ tt)])


def composed_errors(pose, pose1, pose2):
    """The pose of view 2 found on TwoViewPose's landmarks (baseline 1) against ground truth: the rotation's angle, and the camera position
    scaled back by the true baseline of views 0 and 1."""
    scale = np.linalg.norm(pose1[0].T @ pose1[1])
    Rm, _, p = _pose64(pose)
    return _angle(Rm, pose2[0]), float(np.linalg.norm(p * scale + pose2[0].T @ pose2[1]))


# ---- the checks, each over a way to call the restatement (the contract, or a mutant) ---------------------------------------------------

def check_float64(solve):
    """The final pose and statuses against the float64 restatement on the family with 30 % outliers, noise-free and at 0.3 px, threshold
    0.5 px (at 0.3 px noise some inliers fail it), and on a pose per quaternion branch through a camera with fx != fy."""
    worst = np.zeros(2)
    cases = [(name, noise, R.K) for name in R.FAMILY for noise in NOISES] + [(name, 0.3, R.K_OTHER) for name in R.SHEPPERD_POSES]
    for name, noise, K in cases:
        X, uv, _, _ = R.family_scene(name, 300, 1, noise, 0.3, K)
        r, r64 = solve(X, uv, _status(300), K=K, threshold=0.5), R64.solve(X, uv, _status(300), K, threshold=0.5)
        assert int(r.valid[0]) == 1 and r64.valid == 1, (name, noise)
        Rm, _, p = _pose64(r.pose)
        dev = np.array([_angle(Rm, r64.R), np.linalg.norm(p + r64.R.T @ r64.t)])
        worst = np.maximum(worst, dev)
        assert dev[0] <= ROTATION_TOLERANCE and dev[1] <= POSITION_TOLERANCE, (name, noise, dev)
        assert abs(np.linalg.norm(r.pose[:4].astype(np.float64)) - 1.0) <= 1e-6 and r.pose[0] >= 0
        kept = r.status == R.TRACKED
        band = MARGIN_MULTIPLE * float(np.float32(K[0])) * (MEASURED[0] + MEASURED[1] / MIN_DEPTH)
        differ = np.flatnonzero(kept != r64.kept)
        assert (np.abs(r64.margin[differ]) <= band).all(), (name, noise, r64.margin[differ])
        assert int(r.n_inliers[0]) == int(kept.sum()) and (r.status[~kept] == R.LARGE_RESIDUAL).all()
    return worst


def check_ground_truth(solve):
    """The final pose against the scene's own on the family with 30 % outliers.  Returns the worst errors per noise."""
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


def check_stage4(solve):
    """The winner's pose before any refit step against ground truth, noise-free and without outliers."""
    worst = np.zeros(2)
    for name in R.FAMILY:
        X, uv, _, truth = R.family_scene(name, 300, 1)
        r = solve(X, uv, _status(300), refine_iterations=0)
        assert int(r.valid[0]) == 1
        err = _truth_errors(r.pose, truth)
        worst = np.maximum(worst, err)
        assert (err <= STAGE4_TOLERANCE).all(), (name, err)
    return worst


def check_every_hypothesis_counts_its_sample(solve):
    """Noise-free and without outliers, at 1 px: a valid hypothesis counts every participant it can see in front, its six among them."""
    for name in R.SHEPPERD_POSES:
        X, uv, _, _ = R.family_scene(name, 300, 1)
        r = solve(X, uv, _status(300))
        assert (r.counts >= 0).sum() >= 400 and (r.counts[r.counts >= 0] >= R.SAMPLE).all(), name
    X, uv, status, truth = R.wide_case()  # every model's sign is fixed here
    r = solve(X, uv, status, K=R.K_WIDE)
    assert (r.counts >= 0).sum() >= 400 and (r.counts[r.counts >= 0] >= R.SAMPLE).all() and int(r.n_inliers[0]) == 64
    assert (_truth_errors(r.pose, truth) <= (1e-3, 1e-2)).all()  # (loose: this case is about the sign)


def check_separation(solve):
    """At 300 points, 30 % gross outliers, 512 hypotheses and 1 px: without noise every true inlier and no outlier is kept; at 0.3 px noise
    no outlier is kept."""
    for name in SEPARATION_POSES:
        for noise in NOISES:
            X, uv, is_inlier, _ = R.family_scene(name, 300, 1, noise, 0.3)
            r = solve(X, uv, _status(300), hypotheses=512, threshold=1.0)
            kept = r.status == R.TRACKED
            assert not kept[~is_inlier].any(), (name, noise)
            if noise == 0.0:
                assert kept[is_inlier].all(), (name, int(kept.sum()))


def _tree_sums(X, uv, status, pose, model, K=R.K, threshold=1.0):
    """The first refit step's 27 sums by the stated tree, restated apart in numpy float32 from the pose of refine_iterations = 0."""
    f = np.float32
    k = np.array(K, f)
    ry, tn = k[1] / k[0], f(threshold) / k[0]
    tn2 = tn * tn
    x, y = (uv[:, 0] - k[2]) / k[0], (uv[:, 1] - k[3]) / k[1]
    w, qx, qy, qz = (f(v) for v in pose[:4])
    one, two = f(1), f(2)
    Rm = [one - two * (qy * qy + qz * qz), two * (qx * qy - w * qz), two * (qx * qz + w * qy),
          two * (qx * qy + w * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - w * qx),
          two * (qx * qz - w * qy), two * (qy * qz + w * qx), one - two * (qx * qx + qy * qy)]
    d = [X[:, i] - f(pose[4 + i]) for i in range(3)]
    c = [(Rm[j] * d[0] + Rm[3 + j] * d[1]) + Rm[6 + j] * d[2] for j in range(3)]
    cp = [((f(model[r * 4]) * X[:, 0] + f(model[r * 4 + 1]) * X[:, 1]) + f(model[r * 4 + 2]) * X[:, 2]) + f(model[r * 4 + 3]) for r in range(3)]
    ex, ey = cp[0] - x * cp[2], (cp[1] - y * cp[2]) * ry
    inl = (cp[2] > 0) & (ex * ex + ey * ey <= tn2 * (cp[2] * cp[2])) & (c[2] > 0)  # the first step: the inliers of the model that won
    with np.errstate(all="ignore"):
        iz = one / c[2]
    a, b = c[0] * iz, c[1] * iz
    zero = np.zeros_like(a)
    j1 = [a * b, -(one + a * a), b, -iz, zero, a * iz]
    j2 = [ry * (one + b * b), ry * -(a * b), ry * -a, zero, ry * -iz, ry * (b * iz)]
    r1, r2 = a - x, (b - y) * ry
    terms = [j1[i] * j1[j] + j2[i] * j2[j] for i in range(6) for j in range(i, 6)] + [j1[i] * r1 + j2[i] * r2 for i in range(6)]
    terms = np.where(inl, np.stack(terms), f(0)).astype(f)
    total = np.zeros(R.SUMS, f)
    for base in range(0, len(X), R.TILE):
        tile = np.zeros((R.SUMS, R.TILE), f)
        chunk = terms[:, base:base + R.TILE]
        tile[:, :chunk.shape[1]] = chunk
        stride = R.TILE // 2
        while stride >= 1:
            tile[:, :stride] = tile[:, :stride] + tile[:, stride:2 * stride]
            stride //= 2
        total = total + tile[:, 0]
    return total


def check_tree(solve):
    """The sums are the stated tree's, bit for bit, at M <= 256, one tile and a bit, and five tiles (every row a participant)."""
    for name in ("n7", "n256", "n257", "n1025"):
        X, uv, status = R.case(name)
        start = solve(X, uv, status, refine_iterations=0)
        assert E.same(solve(X, uv, status, refine_iterations=1).sums, _tree_sums(X, uv, status, start.pose, start.models[int(start.best[0])])), name


def check_zero_landmarks(solve):
    """Rows with a (0, 0, 0) landmark and status TRACKED take no part: they keep their status and the result is that of the other rows."""
    X, uv, status = R.case("zeros")
    zero = ~X.any(1)
    assert zero.sum() == 5
    r = solve(X, uv, status)
    others = solve(X[~zero], uv[~zero], status[~zero])
    assert (r.status[zero] == R.TRACKED).all() and E.same(r.pose, others.pose) and int(r.n_inliers[0]) == int(others.n_inliers[0]) == 35


CHECKS = {"sign_of_p_not_fixed": check_every_hypothesis_counts_its_sample, "a_transposed": check_stage4, "sequential_sum": check_tree,
          "y_residual_unscaled": check_float64, "zero_landmark_rule_omitted": check_zero_landmarks}


@pytest.mark.parametrize("check", [check_float64, check_ground_truth, check_stage4, check_every_hypothesis_counts_its_sample, check_separation, check_tree,
                                   check_zero_landmarks], ids=lambda c: c.__name__)
def test_the_restatement_passes(check):
    check(_contract())


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_each_mutant_is_caught(mutant):
    with pytest.raises(AssertionError):
        CHECKS[mutant](_contract(R.MUTANTS[mutant]))


def test_the_tolerances_are_the_measured_deviations_with_their_margin():
    worst, truth, stage4 = check_float64(_contract()), check_ground_truth(_contract()), check_stage4(_contract())
    print(f"against float64: rotation {worst[0]:.3e} rad, position {worst[1]:.3e}; against truth: " +
          "; ".join(f"noise {n}: rotation {truth[n][0]:.3e}, position {truth[n][1]:.3e}" for n in NOISES) +
          f"; before the refit: rotation {stage4[0]:.3e}, position {stage4[1]:.3e}")
    pairs = list(zip((ROTATION_TOLERANCE, POSITION_TOLERANCE), worst)) + list(zip(STAGE4_TOLERANCE, stage4))
    for noise in NOISES:
        pairs += list(zip(TRUTH_TOLERANCE[noise], truth[noise]))
    for tolerance, measured in pairs:
        assert tolerance / 8 <= measured <= tolerance  # no more than 8 x what is measured: it was not set loose


def test_the_three_restatements_composed_find_view_two():
    pose1, pose2 = (R.family_pose(name) for name in COMPOSED_POSES)
    uv0, uv1, uv2, is_inlier, _ = R.three_views(300, 1, pose1, pose2, noise=0.0, outlier_share=0.3)
    filtered = T.ransac(uv0, uv1, _status(300), E.IMAGE, 1.0, 512, 1, "fundamental")
    pose01 = P.solve(uv0, uv1, filtered.status)
    fit = R.solve(pose01.points, uv2, pose01.status, seed=3)
    assert int(pose01.valid[0]) == 1 and int(fit.valid[0]) == 1 and int(fit.n_inliers[0]) >= 150
    assert not (fit.status == R.TRACKED)[~is_inlier].any()
    rotation, position = composed_errors(fit.pose, pose1, pose2)
    print(f"view 2 against truth: rotation {rotation:.3e} rad, position {position:.3e}")
    for tolerance, measured in ((COMPOSED_ROTATION_TOLERANCE, rotation), (COMPOSED_POSITION_TOLERANCE, position)):
        assert tolerance / 8 <= measured <= tolerance


# ---- edges --------------------------------------------------------------------------------------------------------------------------------

def _invalid(r, status):
    return (int(r.valid[0]) == -1 and np.array_equal(r.pose, np.array([1, 0, 0, 0, 0, 0, 0], np.float32)) and int(r.n_inliers[0]) == 0
            and int(r.best[0]) == -1 and np.array_equal(r.status, status))


def test_few_participants():
    for m, valid in ((5, False), (6, True), (7, True)):
        X, uv, status = R.case(f"n{m}")
        r = R.solve(X, uv, status)
        assert _invalid(r, status) and (r.counts == -1).all() if not valid else int(r.valid[0]) == 1 and int(r.n_inliers[0]) == m


@pytest.mark.parametrize("name", ["identical", "coplanar"])
def test_degenerate_landmarks_are_invalid(name):
    X, uv, status = R.case(name)
    for threshold in (1.0, 0.0):
        r = R.solve(X, uv, status, threshold=threshold)
        assert _invalid(r, status) and (r.counts == -1).all() and not r.models.any(), name


def test_hostile_rows_take_no_part_unless_finite():
    X, uv, status = R.case("hostile")
    finite = np.isfinite(X).all(1) & np.isfinite(uv).all(1)
    r = R.solve(X, uv, status)
    assert int(r.valid[0]) == 1 and (r.status[~finite] == R.TRACKED).all()  # NaN and inf: no participant, not touched
    huge = finite & ((np.abs(X) > 1e29).any(1) | (np.abs(uv) > 1e29).any(1))
    assert huge.sum() == 3 and (r.status[huge] == R.LARGE_RESIDUAL).all()  # 1e30 is finite: a participant, and no inlier
    assert np.isfinite(r.pose).all() and int(r.n_inliers[0]) == int((finite & ~huge).sum())


def test_landmarks_behind_the_camera_end_the_refit_at_its_first_step():
    X, uv, status = R.case("behind")
    r = R.solve(X, uv, status)
    assert r.trace[R.TRACE_DET_NEGATIVE] == 1 and r.trace[R.TRACE_STEP0] == R.STEP_FEW_INLIERS and r.trace[R.TRACE_STEPS] == 0
    assert int(r.valid[0]) == 1 and int(r.n_inliers[0]) == 0 and (r.status == R.LARGE_RESIDUAL).all()


def test_a_refit_that_ends_early_after_a_step():
    """A threshold so tight that the winner's inliers carry one step and the pose after it keeps fewer than six."""
    X, uv, _, _ = R.scene(300, 2, noise=0.3)
    r = R.solve(X, uv, _status(300), threshold=EARLY_END_THRESHOLD)
    steps = r.trace[R.TRACE_STEP0:R.TRACE_STEP0 + 4].tolist()
    assert int(r.valid[0]) == 1 and r.trace[R.TRACE_STEPS] >= 1 and R.STEP_FEW_INLIERS in steps, steps
    # the pose before the step that ended the refit stands
    assert E.same(r.pose, R.solve(X, uv, _status(300), threshold=EARLY_END_THRESHOLD, refine_iterations=int(r.trace[R.TRACE_STEPS])).pose)


EARLY_END_THRESHOLD = 0.03  # pixels, at 0.3 px noise: the winner counts 7, one step is taken, the pose after it keeps fewer than 6


def test_refine_iterations_zero_returns_the_winners_pose_and_more_steps_do_not_move_a_converged_pose_far():
    X, uv, _, truth = R.scene(300, 2, noise=0.3, outlier_share=0.3)
    errors = [_truth_errors(R.solve(X, uv, _status(300), refine_iterations=k).pose, truth) for k in (0, 1, 4, 16)]
    assert errors[2][0] < errors[0][0] and errors[2][1] < errors[0][1]  # the refit improves on the six-point pose
    assert np.abs(errors[3] - errors[2]).max() <= 1e-5


def test_non_participants_are_not_read_and_not_touched():
    X, uv, status = R.case("n64_half")
    out = status != R.TRACKED
    X2, uv2 = X.copy(), uv.copy()
    X2[out], uv2[out] = np.nan, np.nan
    a, b = R.solve(X, uv, status), R.solve(X2, uv2, status)
    assert R.same_results(a, b, R.OUTPUTS + R.HYPOTHESES) == [] and np.array_equal(a.status[out], status[out]) and int(a.valid[0]) == 1


def test_two_calls_give_equal_bits_and_the_seed_matters():
    X, uv, _, _ = R.scene(300, 2, noise=0.3, outlier_share=0.3)
    a, b, c = (R.solve(X, uv, _status(300), seed=s) for s in (4, 4, 5))
    assert R.same_results(a, b, R.OUTPUTS + R.HYPOTHESES) == [] and "models" in R.same_results(a, c, R.HYPOTHESES)


def test_the_family_reaches_every_branch_of_the_quaternion_and_both_outcomes_of_the_negation():
    traces = np.array([R.solve(*R.family_case(name)).trace for name in R.FAMILY])
    assert set(traces[:, R.TRACE_SHEPPERD]) == {0, 1, 2, 3} and set(traces[:, R.TRACE_NEGATED]) == {0, 1}
    assert (traces[:, R.TRACE_WINNER] >= 0).all() and (traces[:, R.TRACE_STEPS] == 4).all() and (traces[:, R.TRACE_DET_NEGATIVE] == 0).all()
    for name, trace in zip(R.FAMILY, traces):
        assert trace[R.TRACE_SHEPPERD] == P.SHEPPERD_BRANCH[name.split("/")[0]], name


def test_the_threshold_is_in_pixels_with_unequal_focal_lengths():
    """fx != fy: a row's verdict is that of its reprojection error in pixels (float64), except within a thousandth of a pixel of the threshold."""
    X, uv, _, _ = R.family_scene("small/side", 300, 1, 0.3, 0.0, R.K_OTHER)
    r = R.solve(X, uv, _status(300), K=R.K_OTHER, threshold=0.5)
    Rm, t, _ = _pose64(r.pose)
    Y = X.astype(np.float64) @ Rm.T + t
    k = [float(np.float32(v)) for v in R.K_OTHER]
    err = np.hypot(k[0] * Y[:, 0] / Y[:, 2] + k[2] - uv[:, 0], k[1] * Y[:, 1] / Y[:, 2] + k[3] - uv[:, 1])
    kept = r.status == R.TRACKED
    sure = np.abs(err - 0.5) > 1e-3
    assert (kept[sure] == (err[sure] <= 0.5)).all() and 50 <= kept.sum() < 300
