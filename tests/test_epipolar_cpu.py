"""The restatement of two-view outlier rejection (tests/epipolar_ref.c) pinned without a device: synthetic two-view scenes,
an independent float64 null vector by SVD for every hypothesis, the sampler restated apart in Python, the edge cases of the contract, and
five mutants that the same checks must each catch.  tests/test_epipolar_gpu.py then holds the kernels to the restatement bit for bit."""
import numpy as np
import pytest

from tests import epipolar_ref as E

SEEDS = (1, 2, 3)            # scenes for which the noise-free check holds (checked below, not assumed)
MODEL_TOLERANCE = 1.2e-4     # max |f64 - model| per entry: 4 x the worst deviation measured over SEEDS (3.0e-5), DESIGN.md 5.20
CONDITION_FLOOR = 1.0e-4     # samples with sigma_8 / sigma_1 below it are left out of the float64 pin ...
LEFT_OUT_CAP = 0.02          # ... and may be no more than this share of the valid hypotheses (measured: 0.0052)
NOISY_SHARE = 0.97           # share of true inliers kept / of outliers rejected at 0.3 px noise: measured 1.000 / 1.000, margin 0.03


def _all_tracked(n):
    return np.full(n, E.TRACKED, np.uint8)


# ---- the checks, each over a variant of the restatement (0 = the contract) ---------------------------------------------------------------


def check_noise_free_scenes(variant):
    """Noise-free inliers plus 30 % gross outliers at least 4 px from their epipolar lines, t = 1, K = 512: every inlier kept, every outlier
    rejected."""
    for seed in SEEDS:
        ref, cur, is_inlier, _ = E.scene(300, seed)
        r = E.ransac(ref, cur, _all_tracked(300), E.IMAGE, 1.0, 512, seed, variant)
        kept = r.status == E.TRACKED
        assert r.best >= 0 and np.array_equal(kept, is_inlier), (seed, int((kept & ~is_inlier).sum()), int((~kept & is_inlier).sum()))
        assert r.n_inliers == int(is_inlier.sum()) == r.counts[r.best] and (r.status[~kept] == E.LARGE_RESIDUAL).all()


def check_sampler(variant):
    """The indices of every draw equal the Python restatement of the sampler, exactly; a sample holds 8 distinct participants."""
    for name, K, seed in (("n9", 64, 5), ("n8", 64, 0), ("n257", 63, 0xFFFFFFFF), ("interleaved", 65, 9), ("n64_half", 65, 3)):
        ref, cur, status, image = E.case(name)
        r = E.ransac(ref, cur, status, image, 1.0, K, seed, variant)
        assert np.array_equal(r.samples, E.sample_indices(status, K, seed)), name
        for h in range(K):
            drawn = r.samples[h][r.samples[h] >= 0]
            assert len(set(drawn.tolist())) == len(drawn) and (status[drawn] == E.TRACKED).all(), (name, h)
            assert (len(drawn) == E.SAMPLE) or r.counts[h] == -1, (name, h)


def check_tie(variant):
    """Eight noise-free participants: every valid hypothesis holds the same eight points and counts all eight; the lowest h wins."""
    ref, cur, _, _ = E.scene(8, 11, outlier_share=0.0)
    r = E.ransac(ref, cur, _all_tracked(8), E.IMAGE, 1.0, 64, 0, variant)
    top = np.flatnonzero(r.counts == r.counts.max())
    assert r.counts.max() == 8 and len(top) >= 2 and r.best == top[0] and r.n_inliers == 8


def _f64_models(ref, cur, r, image):
    """Per valid hypothesis: (h, float64 unit null vector of the sample's constraint matrix with the model's sign, sigma_8 / sigma_1)."""
    H, W = image
    cx, cy, s = np.float32(0.5) * np.float32(W - 1), np.float32(0.5) * np.float32(H - 1), np.float32(2.0) / np.float32(W + H)
    centre, s = np.array([cx, cy], np.float64), np.float64(s)
    out = []
    for h in np.flatnonzero(r.counts >= 0):
        x1 = (ref[r.samples[h]].astype(np.float64) - centre) * s
        x2 = (cur[r.samples[h]].astype(np.float64) - centre) * s
        A = np.stack([x2[:, 0] * x1[:, 0], x2[:, 0] * x1[:, 1], x2[:, 0], x2[:, 1] * x1[:, 0], x2[:, 1] * x1[:, 1], x2[:, 1], x1[:, 0], x1[:, 1],
                      np.ones(8)], axis=1)
        _, sv, vt = np.linalg.svd(A)
        f = vt[-1] / np.linalg.norm(vt[-1])
        if f @ r.models[h].astype(np.float64) < 0:
            f = -f
        out.append((h, f, sv[7] / sv[0]))
    return out, centre, s


def check_float64_pin(variant):
    """models against the SVD null vectors, and counts against the float64 classification: a count may differ only by points whose float64
    residual lies within the model's own deviation of the threshold."""
    left_out = total = 0
    worst = 0.0
    for seed in SEEDS:
        ref, cur, _, _ = E.scene(300, seed)
        r = E.ransac(ref, cur, _all_tracked(300), E.IMAGE, 1.0, 512, seed, variant)
        models, centre, s = _f64_models(ref, cur, r, E.IMAGE)
        x1 = (ref.astype(np.float64) - centre) * s
        x2 = (cur.astype(np.float64) - centre) * s
        tn = 1.0 * s
        for h, f, ratio in models:
            total += 1
            if ratio < CONDITION_FLOOR:
                left_out += 1
                continue
            deviation = np.abs(f - r.models[h]).max()
            worst = max(worst, deviation)
            assert deviation <= MODEL_TOLERANCE, (seed, h, deviation, ratio)
            assert abs(np.linalg.norm(r.models[h].astype(np.float64)) - 1.0) <= 1e-6
            F = f.reshape(3, 3)
            a = np.c_[x1, np.ones(300)] @ F.T   # F x1
            b = np.c_[x2, np.ones(300)] @ F     # F^T x2
            num = (np.c_[x2, np.ones(300)] * a).sum(axis=1)
            den = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
            margin = np.abs(num) - tn * np.sqrt(den)
            band = 8.0 * deviation + 2e-6  # |d num| <= |x2|_1 |x1|_1 max|dF| <= 4 max|dF|, as much again for the right-hand side; float32 rounding
            sure_in, near = int((margin < -band).sum()), int((np.abs(margin) <= band).sum())
            assert sure_in <= r.counts[h] <= sure_in + near, (seed, h, sure_in, near, int(r.counts[h]))
    assert total >= 1500 and left_out <= LEFT_OUT_CAP * total, (left_out, total)
    return worst, left_out / total


CHECKS = {"highest_h_on_a_tie": check_tie, "f_applied_transposed": check_float64_pin, "sampler_allows_duplicates": check_sampler,
          "threshold_unscaled": check_noise_free_scenes, "non_participants_sampled": check_sampler}


@pytest.mark.parametrize("check", [check_noise_free_scenes, check_sampler, check_tie, check_float64_pin], ids=lambda c: c.__name__)
def test_the_restatement_passes(check):
    check(E.CONTRACT)


@pytest.mark.parametrize("mutant", sorted(E.MUTANTS))
def test_each_mutant_is_caught(mutant):
    with pytest.raises(AssertionError):
        CHECKS[mutant](E.MUTANTS[mutant])


def test_noisy_scene_shares():
    """0.3 px Gaussian noise on the inliers' current points, t = 1: the shares measured here (1.000 kept, 1.000 rejected over the three
    scenes) hold with the stated margin."""
    for seed in SEEDS:
        ref, cur, is_inlier, _ = E.scene(300, seed, noise=0.3)
        r = E.ransac(ref, cur, _all_tracked(300), E.IMAGE, 1.0, 512, seed)
        kept = r.status == E.TRACKED
        share_kept, share_rejected = (kept & is_inlier).sum() / is_inlier.sum(), (~kept & ~is_inlier).sum() / (~is_inlier).sum()
        print(f"seed {seed}: inliers kept {share_kept:.4f}, outliers rejected {share_rejected:.4f}")
        assert share_kept >= NOISY_SHARE and share_rejected >= NOISY_SHARE


def test_the_tolerance_is_the_measured_deviation_with_its_margin():
    worst, share = check_float64_pin(E.CONTRACT)
    print(f"worst |f64 - model| {worst:.3e}, left out {share:.4f}")
    assert MODEL_TOLERANCE / 8 <= worst  # the tolerance is no more than 8 x what is measured: it was not set loose


@pytest.mark.parametrize("m", [7, 8, 9])
def test_few_participants(m):
    ref, cur, status, image = E.case(f"n{m}")
    r = E.ransac(ref, cur, status, image, 1.0, 64, 1)
    if m < 8:
        assert r.best == -1 and r.n_inliers == m and not r.F.any() and (r.counts == -1).all() and not r.models.any() and np.array_equal(r.status, status)
    else:
        assert r.best >= 0 and (r.counts >= 0).any()
        assert m > 8 or (r.counts == -1).any()  # at M = 8 the last draw has one position left: some samplers run out of attempts
        assert r.n_inliers == r.counts.max() == (r.status == E.TRACKED).sum()


@pytest.mark.parametrize("name", ["identical", "collinear"])
def test_degenerate_points_change_nothing(name):
    ref, cur, status, image = E.case(name)
    r = E.ransac(ref, cur, status, image, 1.0, 64, 0)
    assert r.best == -1 and r.n_inliers == 40 and not r.F.any() and (r.counts == -1).all() and np.array_equal(r.status, status)


def test_hostile_coordinates_are_never_inliers():
    ref, cur, status, image = E.case("hostile")
    r = E.ransac(ref, cur, status, image, 1.0, 256, 0)
    bad = ~(np.isfinite(ref).all(axis=1) & np.isfinite(cur).all(axis=1)) | (np.abs(ref).max(axis=1) > 1e29) | (np.abs(cur).max(axis=1) > 1e29)
    assert bad.sum() == 6 and r.best >= 0 and (r.status[bad] == E.LARGE_RESIDUAL).all() and np.isfinite(r.F).all() and np.isfinite(r.models).all()
    assert (r.status[~bad] == E.TRACKED).sum() == r.n_inliers > 8
    for h in np.flatnonzero(r.counts >= 0):  # a sample with a non-finite point is invalid
        assert not bad[r.samples[h]].any() or np.abs(ref[r.samples[h]]).max() > 1e29 or np.abs(cur[r.samples[h]]).max() > 1e29


def test_one_hypothesis():
    """K = 1: seed 4 draws eight true inliers of scene 1 (checked), so the one hypothesis is valid, wins, and the status rewrite is its count."""
    ref, cur, is_inlier, _ = E.scene(300, 1)
    status = _all_tracked(300)
    r = E.ransac(ref, cur, status, E.IMAGE, 1.0, 1, 4)
    assert np.array_equal(r.samples, E.sample_indices(status, 1, 4)) and (r.samples[0] >= 0).all()
    assert r.counts.shape == (1,) and r.counts[0] >= 8 and r.best == 0 and r.n_inliers == r.counts[0] == (r.status == E.TRACKED).sum()
    assert (r.status[r.samples[0]] == E.TRACKED).all() and (r.status[r.status != E.TRACKED] == E.LARGE_RESIDUAL).all()
    if is_inlier[r.samples[0]].all():  # an all-inlier sample fits the scene: every inlier kept, every outlier rejected
        assert np.array_equal(r.status == E.TRACKED, is_inlier)
    invalid = E.ransac(*E.case("identical")[:3], E.IMAGE, 1.0, 1, 4)  # and the one hypothesis invalid: nothing changes
    assert invalid.best == -1 and invalid.counts[0] == -1 and invalid.n_inliers == 40 and (invalid.status == E.TRACKED).all()


def test_non_participants_are_not_read_and_not_touched():
    ref, cur, status, image = E.case("interleaved")
    r = E.ransac(ref, cur, status, image, 1.0, 128, 2)
    out = status != E.TRACKED
    assert r.best >= 0 and np.array_equal(r.status[out], status[out]) and (status[r.samples[r.samples >= 0]] == E.TRACKED).all()
    ref2 = ref.copy()
    ref2[out] = 12345.0
    r2 = E.ransac(ref2, cur, status, image, 1.0, 128, 2)
    assert E.same(r.status, r2.status) and E.same(r.models, r2.models) and E.same(r.counts, r2.counts) and E.same(r.F, r2.F)


def test_repeat_and_seed():
    ref, cur, _, _ = E.scene(300, 2)
    a, b, c = (E.ransac(ref, cur, _all_tracked(300), E.IMAGE, 1.0, 64, seed) for seed in (7, 7, 8))
    for field in ("status", "F", "counts", "models", "samples"):
        assert E.same(getattr(a, field), getattr(b, field)), field
    assert (a.best, a.n_inliers) == (b.best, b.n_inliers) and not np.array_equal(a.samples, c.samples)


def test_pixel_F_is_the_denormalised_model():
    """F = T^T F_n T: the pixel-unit residuals of the inliers vanish, and x_cur^T F x_ref equals the normalised form to rounding."""
    ref, cur, is_inlier, F_true = E.scene(300, 3)
    r = E.ransac(ref, cur, _all_tracked(300), E.IMAGE, 1.0, 512, 3)
    x1, x2 = np.c_[ref.astype(np.float64), np.ones(300)], np.c_[cur.astype(np.float64), np.ones(300)]
    F = r.F.astype(np.float64)
    line = x1 @ F.T
    distance = np.abs((x2 * line).sum(axis=1)) / np.hypot(line[:, 0], line[:, 1])
    assert distance[is_inlier].max() < 1.0 and distance[~is_inlier].min() > 1.0
    H, W = E.IMAGE
    s, cx, cy = 2.0 / (W + H), 0.5 * (W - 1), 0.5 * (H - 1)
    T = np.array([[s, 0, -cx * s], [0, s, -cy * s], [0, 0, 1]])
    assert np.abs(T.T @ r.models[r.best].astype(np.float64).reshape(3, 3) @ T - F).max() <= 1e-6 * np.abs(F).max()


# ---- more than one camera motion: the pose family of tests/two_view_pose_ref.py -----------------------------------------

EPIPOLE_RADIUS = 20.0  # pixels


def near_the_epipole(pose, ref, cur):
    """Points within EPIPOLE_RADIUS of the epipole in either image (K t / t_z in the current one, K (-R^T t) / (.)_z in the reference)."""
    from tests import two_view_pose_ref as P
    R, t = P.family_pose(pose)
    fx, fy, cx, cy = P.K
    e_cur, e_ref = t, -R.T @ t
    near = np.zeros(len(ref), bool)
    for uv, e in ((cur, e_cur), (ref, e_ref)):
        if abs(e[2]) > 1e-9:
            near |= np.hypot(uv[:, 0] - (fx * e[0] / e[2] + cx), uv[:, 1] - (fy * e[1] / e[2] + cy)) <= EPIPOLE_RADIUS
    return near


def _sampson_pixels(f, ref, cur, image=E.IMAGE, of_pixels=False):
    """The contract's residual of every point under a model of the normalised coordinates (or of pixels), float64, in pixels."""
    H, W = image
    centre, s = (np.zeros(2), 1.0) if of_pixels else (np.array([0.5 * (W - 1), 0.5 * (H - 1)]), 2.0 / (W + H))
    x1, x2 = np.c_[(ref.astype(np.float64) - centre) * s, np.ones(len(ref))], np.c_[(cur.astype(np.float64) - centre) * s, np.ones(len(ref))]
    F = np.asarray(f, np.float64).reshape(3, 3)
    a, b = x1 @ F.T, x2 @ F
    return np.abs((x2 * a).sum(axis=1)) / np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2) / s


KEPT_OUTLIERS = {"small/forward": 1, "z-150/side": 1, "z90/forward": 3}  # at seed 1, 512 hypotheses; every other pose of the family: none


def family_filter_runs():
    """(pose, ref_uv, cur_uv, is_inlier, the restatement's result, float64's eigenvalue ratio of the inliers' A) over the whole family at 300
    points, 30 % outliers, seed 1, 512 hypotheses."""
    from tests import two_view_pose_ref as P
    from tests.test_two_view_pose_cpu import _rank_ratio64
    for pose in P.FAMILY:
        ref, cur, is_inlier, _ = P.family_scene(pose, 300, 1, outlier_share=0.3)
        r = E.ransac(ref, cur, _all_tracked(300), E.IMAGE, 1.0, 512, 1)
        yield pose, ref, cur, is_inlier, r, _rank_ratio64(ref, cur, np.where(is_inlier, E.TRACKED, E.OUTSIDE).astype(np.uint8))


def test_the_pose_family_is_cleaned_as_far_as_its_scenes_determine_one_model():
    """The whole pose family.  No inlier is ever rejected, those within 20 px of an epipole included.  check_noise_free_scenes' other half,
    every outlier rejected, holds where the scene determines one fundamental matrix: float64's ratio of the second-smallest to the largest
    eigenvalue of the inliers' A at or above P.FILTER_WELL_CONDITIONED (14 poses).  Below it (the small turns and the turns about z of a
    shallow cube: 1.6e-6 ... 6.6e-6) the second eigenvector fits the inliers to 0.9 ... 4.6 px rms, a mix of the two still fits all of them
    within the pixel, and a sample of seven inliers and an outlier picks the mix through that outlier: it counts one more than any clean
    sample and wins, as the greatest count must.  On three poses that happens; it is shown to be the scene and not the arithmetic: the winning
    sample holds the kept outlier, the float64 null vector of the same sample keeps it too (at 0.0 px) with every inlier, and under the true F
    it lies 19 px (small/forward), 4.1 px (z-150/side) and 1.4 ... 2.8 px (z90/forward) away.  A refit on the inliers is not part of 5.20."""
    from tests import two_view_pose_ref as P
    seen, near_total = {}, 0
    for pose, ref, cur, is_inlier, r, ratio in family_filter_runs():
        kept = r.status == E.TRACKED
        wrong = kept & ~is_inlier
        assert r.best >= 0 and kept[is_inlier].all(), (pose, int((~kept & is_inlier).sum()))
        assert r.n_inliers == int(kept.sum()) == r.counts[r.best] and (r.status[~kept] == E.LARGE_RESIDUAL).all()
        if pose.endswith("/forward"):
            near = near_the_epipole(pose, ref, cur) & is_inlier
            near_total += int(near.sum())
            assert kept[near].all(), pose
        if ratio >= P.FILTER_WELL_CONDITIONED:
            assert not wrong.any(), (pose, ratio, np.flatnonzero(wrong))
        if wrong.any():
            seen[pose] = int(wrong.sum())
            models, _, _ = _f64_models(ref, cur, r, E.IMAGE)
            f64 = next(f for h, f, _ in models if h == r.best)
            distance = _sampson_pixels(f64, ref, cur)
            assert set(np.flatnonzero(wrong)) & set(r.samples[r.best].tolist()), pose       # the winning sample holds a kept outlier
            assert (distance[kept] <= 1.0).all() and (distance[~kept] > 1.0).all(), pose      # float64 on that sample: the same verdict
            assert (_sampson_pixels(P.family_scene(pose, 300, 1, outlier_share=0.3)[3], ref, cur, of_pixels=True)[wrong] > 1.0).all(), pose
    assert seen == KEPT_OUTLIERS, seen
    assert near_total >= 3  # x170/forward, y170/forward and z90/forward have inliers about the epipole
