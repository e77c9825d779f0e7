"""The restatement of two-view outlier rejection with a choice of model (tests/two_view_ref.c) pinned without a device:
mode 0 against tests/epipolar_ref.c bit for bit, the homography sampler restated apart in Python, an independent float64 null vector by SVD
for every homography hypothesis, the planar scenes with a moving patch (A) and the depth scenes (B), the rule and its edge cases, and five
mutants that the same checks must each catch.  tests/test_two_view_gpu.py then holds the kernels to the restatement bit for bit."""
import numpy as np
import pytest

from tests import epipolar_ref as E
from tests import two_view_ref as T

SEEDS = (1, 2, 3)
MODEL_TOLERANCE = 1.43e-4    # max |h64 - model| per entry: 4 x the worst deviation measured over scenes A and B, SEEDS (3.57e-5), DESIGN.md 5.21
CONDITION_FLOOR = 1.0e-4     # samples with sigma_8 / sigma_1 below it are left out of the float64 pin ...
LEFT_OUT_CAP = 0.02          # ... and may be no more than this share of the valid hypotheses (measured: 0.0042; 0.0085 on scene A alone)
BACKGROUND_CAP = 1.0 / 20    # share of background points a homography may reject at 0.3 px noise (measured: at most 5 of 255 = 0.0196)
PREFER = 750


def _all_tracked(n):
    return np.full(n, T.TRACKED, np.uint8)


def _scene_a(seed, camera, noise):
    ref, cur, on_patch, _ = T.planar_scene(300, seed, camera, noise)
    return ref, cur, on_patch


# ---- the checks, each over a variant of the restatement (0 = the contract) ---------------------------------------------------------------


def check_mode_0_is_the_epipolar_restatement(variant):
    """Mode 0 equals tests/epipolar_ref.c bit for bit; slot 1 holds what a model that did not run holds."""
    cases = [(name, K, 3) for name in ("n7", "n8", "n9", "n64_half", "n257") for K in (1, 65)] + [(name, 64, 0) for name in E.HOSTILE_CASES]
    for name, K, seed in cases:
        ref, cur, status, image = E.case(name)
        want = E.ransac(ref, cur, status, image, 1.0, K, seed)
        r = T.ransac(ref, cur, status, image, 1.0, K, seed, T.FUNDAMENTAL, PREFER, variant)
        for field, got in (("status", r.status), ("F", r.F), ("counts", r.counts[0]), ("models", r.models[0]), ("samples", r.samples_f)):
            assert E.same(got, getattr(want, field)), (name, K, field)
        assert (int(r.best[0]), int(r.n_inliers[0])) == (want.best, want.n_inliers) and r.model == (0 if want.best >= 0 else -1), (name, K)
        m = int((status == T.TRACKED).sum())
        assert r.best[1] == -1 and r.n_inliers[1] == m and not r.H.any() and (r.counts[1] == -1).all() and not r.models[1].any(), (name, K)


def check_homography_sampler(variant):
    """The indices of every homography draw equal the Python restatement of the sampler, exactly; a sample holds 4 distinct participants."""
    for name, K, seed in (("n4", 64, 5), ("n5", 64, 0), ("n9", 64, 1), ("n257", 63, 0xFFFFFFFF), ("interleaved", 65, 9), ("n64_half", 65, 3)):
        ref, cur, status, image = T.case(name)
        r = T.ransac(ref, cur, status, image, 1.0, K, seed, T.HOMOGRAPHY, PREFER, variant)
        assert np.array_equal(r.samples_h, T.sample_indices(status, K, seed)), name
        for h in range(K):
            drawn = r.samples_h[h][r.samples_h[h] >= 0]
            assert len(set(drawn.tolist())) == len(drawn) and (status[drawn] == T.TRACKED).all(), (name, h)
            assert (len(drawn) == T.H_SAMPLE) or r.counts[1, h] == -1, (name, h)


def _h64_models(ref, cur, r, image):
    """Per valid homography hypothesis: (h, float64 unit null vector of the sample's DLT system with the model's sign, sigma_8 / sigma_1)."""
    H, W = image
    cx, cy, s = np.float32(0.5) * np.float32(W - 1), np.float32(0.5) * np.float32(H - 1), np.float32(2.0) / np.float32(W + H)
    centre, s = np.array([cx, cy], np.float64), np.float64(s)
    out = []
    for h in np.flatnonzero(r.counts[1] >= 0):
        x1 = (ref[r.samples_h[h]].astype(np.float64) - centre) * s
        x2 = (cur[r.samples_h[h]].astype(np.float64) - centre) * s
        rows = []
        for (a, b), (c, d) in zip(x1, x2):
            rows += [[a, b, 1, 0, 0, 0, -c * a, -c * b, -c], [0, 0, 0, a, b, 1, -d * a, -d * b, -d]]
        _, sv, vt = np.linalg.svd(np.array(rows))
        g = vt[-1] / np.linalg.norm(vt[-1])
        if g @ r.models[1, h].astype(np.float64) < 0:
            g = -g
        out.append((h, g, sv[7] / sv[0]))
    return out, centre, s


def check_float64_pin(variant):
    """Homography models against the SVD null vectors, and counts against the float64 classification: a count may differ only by points
    whose float64 residual lies within the model's own deviation of the threshold."""
    left_out = total = 0
    worst = 0.0
    for scene in ("A", "B"):
        for seed in SEEDS:
            ref, cur = _scene_a(seed, "moving", 0.3)[:2] if scene == "A" else E.scene(300, seed)[:2]
            r = T.ransac(ref, cur, _all_tracked(300), T.IMAGE, 1.0, 512, seed, T.HOMOGRAPHY, PREFER, variant)
            models, centre, s = _h64_models(ref, cur, r, T.IMAGE)
            x1 = np.c_[(ref.astype(np.float64) - centre) * s, np.ones(300)]
            x2 = (cur.astype(np.float64) - centre) * s
            tn = 1.0 * s
            for h, g, ratio in models:
                total += 1
                if ratio < CONDITION_FLOOR:
                    left_out += 1
                    continue
                deviation = np.abs(g - r.models[1, h]).max()
                worst = max(worst, deviation)
                assert deviation <= MODEL_TOLERANCE, (scene, seed, h, deviation, ratio)
                assert abs(np.linalg.norm(r.models[1, h].astype(np.float64)) - 1.0) <= 1e-6
                p = x1 @ g.reshape(3, 3).T
                e = p[:, :2] - x2 * p[:, 2:]
                margin = np.hypot(e[:, 0], e[:, 1]) - tn * np.abs(p[:, 2])
                # |d px|, |d py|, |d w| <= (|x1| + |y1| + 1) max|dH| <= 2 max|dH| (normalised |x| <= 0.58, |y| <= 0.43); |d ex| <= |d px| + |x2| |d w|
                # <= 3.2 max|dH|, the same for ey: |d |e|| <= 4.6 max|dH|; the right-hand side moves by tn |d w|, far less; float32 rounding
                band = 6.0 * deviation + 2e-6
                sure_in, near = int((margin < -band).sum()), int((np.abs(margin) <= band).sum())
                assert sure_in <= r.counts[1, h] <= sure_in + near, (scene, seed, h, sure_in, near, int(r.counts[1, h]))
    assert total >= 3000 and left_out <= LEFT_OUT_CAP * total, (left_out, total)
    return worst, left_out / total


def check_scene_a(variant, report=None):
    """Scene A, seeds 1-3, moving and static camera: without noise the homography and auto reject every patch point and no background
    point; at 0.3 px every patch point and at most 1 in 20 background points; auto reports model 1; the fundamental matrix alone rejects
    fewer patch points than the homography."""
    for camera in ("moving", "static"):
        for noise in (0.0, 0.3):
            for seed in SEEDS:
                ref, cur, on_patch = _scene_a(seed, camera, noise)
                status = _all_tracked(300)
                runs = {mode: T.ransac(ref, cur, status, T.IMAGE, 1.0, 512, seed, mode, PREFER, variant) for mode in ("fundamental", "homography", "auto")}
                for mode in ("homography", "auto"):
                    rejected = runs[mode].status == T.LARGE_RESIDUAL
                    on, off = int((rejected & on_patch).sum()), int((rejected & ~on_patch).sum())
                    assert on == int(on_patch.sum()) == 45, (camera, noise, seed, mode, on)
                    assert off == 0 if noise == 0.0 else off <= BACKGROUND_CAP * int((~on_patch).sum()), (camera, noise, seed, mode, off)
                    assert runs[mode].n_inliers[1] == 300 - on - off == int((runs[mode].status == T.TRACKED).sum())
                auto = runs["auto"]
                assert auto.model == 1
                assert E.same(auto.status, runs["homography"].status) and E.same(auto.H, runs["homography"].H)
                assert E.same(auto.F, runs["fundamental"].F) and E.same(auto.counts[0], runs["fundamental"].counts[0])
                assert int(((runs["fundamental"].status == T.LARGE_RESIDUAL) & on_patch).sum()) < 45
                if report is not None:
                    report.append((camera, noise, seed, off, int(auto.n_inliers[1]), int(auto.n_inliers[0])))


def check_scene_b(variant, report=None):
    """Scene B (tests/epipolar_ref.py's scene(), depth 2-10, 30 % gross outliers): auto reports model 0 and its statuses are mode 0's."""
    for seed in SEEDS:
        ref, cur, is_inlier, _ = E.scene(300, seed)
        status = _all_tracked(300)
        auto = T.ransac(ref, cur, status, T.IMAGE, 1.0, 512, seed, T.AUTO, PREFER, variant)
        fundamental = T.ransac(ref, cur, status, T.IMAGE, 1.0, 512, seed, T.FUNDAMENTAL, PREFER, variant)
        assert auto.model == 0 and E.same(auto.status, fundamental.status) and np.array_equal(auto.status == T.TRACKED, is_inlier), seed
        assert E.same(auto.F, fundamental.F) and auto.best[0] == fundamental.best[0] and auto.best[1] >= 0 and auto.H.any()
        if report is not None:
            report.append(("B", seed, int(auto.n_inliers[1]), int(auto.n_inliers[0])))


def check_the_ratios_lie_on_opposite_sides(variant):
    """n_H / n_F on A (every camera and noise) lies above the default 0.75, on B below it."""
    a, b = [], []
    check_scene_a(variant, a)
    check_scene_b(variant, b)
    ratios_a, ratios_b = [n_h / n_f for *_, n_h, n_f in a], [n_h / n_f for *_, n_h, n_f in b]
    assert min(ratios_a) > 0.75 > max(ratios_b), (ratios_a, ratios_b)
    return (min(ratios_a), max(ratios_a)), (min(ratios_b), max(ratios_b)), max(off for _, noise, _, off, _, _ in a if noise > 0) / 255.0


def check_the_rule(variant):
    """The rule on integers, and a constructed tie 1000 n_H == p n_F: scene(20, 301) without outliers, K = 256, seed 1 gives n_F = 20 and
    n_H = 5 (checked), so p = 250 is the tie and chooses the homography, p = 251 the fundamental matrix."""
    for has_f, has_h, n_f, n_h, p, want in ((1, 1, 20, 5, 250, 1), (1, 1, 20, 5, 251, 0), (1, 1, 300, 255, 750, 1), (1, 1, 210, 15, 750, 0), (0, 1, 5, 4, 1000, 1),
                                            (1, 0, 9, 9, 0, 0), (0, 0, 3, 3, 0, -1), (1, 1, 65536, 65535, 1000, 0), (1, 1, 65536, 65536, 1000, 1),
                                            (1, 1, 8, 0, 0, 1)):
        assert T.choose(has_f, has_h, n_f, n_h, p, variant) == want, (has_f, has_h, n_f, n_h, p)
    ref, cur, _, _ = E.scene(20, 301, outlier_share=0.0)
    status = _all_tracked(20)
    at, above = (T.ransac(ref, cur, status, T.IMAGE, 1.0, 256, 1, T.AUTO, p, variant) for p in (250, 251))
    assert (at.n_inliers.tolist(), above.n_inliers.tolist()) == ([20, 5], [20, 5]) and at.best[0] >= 0 and at.best[1] >= 0
    assert at.model == 1 and int((at.status == T.TRACKED).sum()) == 5
    assert above.model == 0 and int((above.status == T.TRACKED).sum()) == 20


def check_the_rewrite_uses_the_chosen_model(variant):
    """After auto, the participants still TRACKED number n_inliers of the chosen model, on A (the homography) and on B (the fundamental matrix)."""
    for ref, cur in (_scene_a(1, "moving", 0.3)[:2], E.scene(300, 1)[:2]):
        r = T.ransac(ref, cur, _all_tracked(300), T.IMAGE, 1.0, 512, 1, T.AUTO, PREFER, variant)
        assert r.model >= 0 and int((r.status == T.TRACKED).sum()) == r.n_inliers[r.model] == r.counts[r.model, r.best[r.model]]


def check_pixel_h(variant):
    """H = T^-1 H_n T: in pixels the inliers' transfer error is below the threshold, the rejected points' above it."""
    ref, cur, on_patch = _scene_a(2, "moving", 0.0)
    r = T.ransac(ref, cur, _all_tracked(300), T.IMAGE, 1.0, 512, 2, T.HOMOGRAPHY, PREFER, variant)
    p = np.c_[ref.astype(np.float64), np.ones(300)] @ r.H.astype(np.float64).T
    error = np.hypot(*(p[:, :2] / p[:, 2:] - cur).T)
    assert error[~on_patch].max() < 1.0 < error[on_patch].min() and np.array_equal(r.status == T.LARGE_RESIDUAL, on_patch)
    H, W = T.IMAGE
    s, cx, cy = 2.0 / (W + H), 0.5 * (W - 1), 0.5 * (H - 1)
    Tn = np.array([[s, 0, -cx * s], [0, s, -cy * s], [0, 0, 1]])
    want = np.linalg.inv(Tn) @ r.models[1, r.best[1]].astype(np.float64).reshape(3, 3) @ Tn
    assert np.abs(want - r.H).max() <= 1e-5 * np.abs(want).max()


CHECKS = {"transfer_error_with_h_transposed": check_float64_pin, "dlt_rows_wrong_sign": check_float64_pin, "auto_rule_counts_swapped": check_the_rule,
          "rewrite_with_the_loser": check_the_rewrite_uses_the_chosen_model, "homography_sampler_allows_duplicates": check_homography_sampler}
ALL_CHECKS = [check_mode_0_is_the_epipolar_restatement, check_homography_sampler, check_float64_pin, check_scene_a, check_scene_b,
              check_the_ratios_lie_on_opposite_sides, check_the_rule, check_the_rewrite_uses_the_chosen_model, check_pixel_h]


@pytest.mark.parametrize("check", ALL_CHECKS, ids=lambda c: c.__name__)
def test_the_restatement_passes(check):
    check(T.CONTRACT)


@pytest.mark.parametrize("mutant", sorted(T.MUTANTS))
def test_each_mutant_is_caught(mutant):
    with pytest.raises(AssertionError):
        CHECKS[mutant](T.MUTANTS[mutant])


def test_the_measured_figures():
    """What DESIGN.md 5.21 records, printed: the worst deviation with the share left out, and the ratios n_H / n_F of scenes A and B."""
    worst, share = check_float64_pin(T.CONTRACT)
    a, b, background = check_the_ratios_lie_on_opposite_sides(T.CONTRACT)
    print(f"worst |h64 - model| {worst:.3e}, left out {share:.4f}; n_H / n_F on A {a[0]:.3f} .. {a[1]:.3f}, on B {b[0]:.3f} .. {b[1]:.3f}; "
          f"background rejected at 0.3 px at most {background:.4f}")
    assert MODEL_TOLERANCE / 8 <= worst  # the tolerance is no more than 8 x what is measured: it was not set loose


@pytest.mark.parametrize("m", [3, 4, 5, 7, 8, 9])
def test_few_participants(m):
    ref, cur, status, image = T.case(f"n{m}")
    for mode in ("fundamental", "homography", "auto"):
        r = T.ransac(ref, cur, status, image, 1.0, 64, 1, mode)
        if m < 8:
            assert r.best[0] == -1 and r.n_inliers[0] == m and not r.F.any() and (r.counts[0] == -1).all() and not r.models[0].any()
        if m < 4 or mode == "fundamental":
            assert r.best[1] == -1 and r.n_inliers[1] == m and not r.H.any() and (r.counts[1] == -1).all() and not r.models[1].any()
        if m < 4 or (m < 8 and mode == "fundamental"):
            assert r.model == -1 and np.array_equal(r.status, status)
        elif m < 8 and mode == "auto":  # at 4 .. 7 only the homography can win
            assert r.model == 1 and r.best[1] >= 0 and r.n_inliers[1] == r.counts[1].max() == (r.status == T.TRACKED).sum() >= 4
        elif mode != "fundamental":
            assert r.best[1] >= 0 and r.n_inliers[1] == r.counts[1].max() and r.model in (0, 1)
            assert (r.status == T.TRACKED).sum() == r.n_inliers[r.model]
        if m == 4 and mode != "fundamental":
            assert (r.counts[1] == -1).any()  # the last draw has one position left: some samplers run out of attempts


@pytest.mark.parametrize("name", ["identical", "collinear"])
def test_degenerate_points_change_nothing(name):
    ref, cur, status, image = T.case(name)
    for mode in ("homography", "auto"):
        r = T.ransac(ref, cur, status, image, 1.0, 64, 0, mode)
        assert r.model == -1 and (r.best == -1).all() and (r.n_inliers == 40).all() and not r.H.any() and not r.F.any()
        assert (r.counts == -1).all() and not r.models.any() and np.array_equal(r.status, status)


def test_hostile_coordinates_are_never_inliers():
    ref, cur, status, image = T.case("hostile")
    bad = ~(np.isfinite(ref).all(axis=1) & np.isfinite(cur).all(axis=1)) | (np.abs(ref).max(axis=1) > 1e29) | (np.abs(cur).max(axis=1) > 1e29)
    for mode in ("homography", "auto"):
        r = T.ransac(ref, cur, status, image, 1.0, 256, 0, mode)
        assert bad.sum() == 6 and r.model >= 0 and (r.status[bad] == T.LARGE_RESIDUAL).all()
        assert np.isfinite(r.F).all() and np.isfinite(r.H).all() and np.isfinite(r.models).all()
        assert (r.status[~bad] == T.TRACKED).sum() == r.n_inliers[r.model]
        for h in np.flatnonzero(r.counts[1] >= 0):  # a sample with a non-finite point is invalid
            assert np.isfinite(ref[r.samples_h[h]]).all() and np.isfinite(cur[r.samples_h[h]]).all()


def test_non_participants_are_not_read_and_not_touched():
    ref, cur, status, image = T.case("interleaved")
    out = status != T.TRACKED
    ref2 = ref.copy()
    ref2[out] = 12345.0
    for mode in ("homography", "auto"):
        r, r2 = (T.ransac(x, cur, status, image, 1.0, 128, 2, mode) for x in (ref, ref2))
        assert r.model >= 0 and np.array_equal(r.status[out], status[out]) and (status[r.samples_h[r.samples_h >= 0]] == T.TRACKED).all()
        assert T.same_results(r, r2) == []


def test_one_hypothesis():
    """K = 1 on a planar scene without noise: seed 0 draws four background points (checked), so the one hypothesis is the plane's."""
    ref, cur, on_patch = _scene_a(1, "moving", 0.0)
    status = _all_tracked(300)
    seed = next(s for s in range(64) if not on_patch[T.sample_indices(status, 1, s)[0]].any())
    for mode in ("homography", "auto"):
        r = T.ransac(ref, cur, status, T.IMAGE, 1.0, 1, seed, mode)
        assert np.array_equal(r.samples_h, T.sample_indices(status, 1, seed)) and r.counts.shape == (2, 1) and r.best[1] == 0 and r.model == 1
        assert np.array_equal(r.status == T.LARGE_RESIDUAL, on_patch) and r.n_inliers[1] == r.counts[1, 0] == 255
    invalid = T.ransac(*T.case("identical")[:3], T.IMAGE, 1.0, 1, 4, T.AUTO)  # and the one hypothesis invalid: nothing changes
    assert invalid.model == -1 and (invalid.counts == -1).all() and (invalid.n_inliers == 40).all() and (invalid.status == T.TRACKED).all()


def test_the_preference_at_its_bounds():
    """p = 0: the homography whenever it has a winner; p = 1000: only when it explains as much as the fundamental matrix."""
    ref, cur, _, _ = E.scene(300, 1)  # B: n_H far below n_F
    status = _all_tracked(300)
    low, high = (T.ransac(ref, cur, status, T.IMAGE, 1.0, 512, 1, T.AUTO, p) for p in (0, 1000))
    assert low.model == 1 and (low.status == T.TRACKED).sum() == low.n_inliers[1] < low.n_inliers[0]
    assert high.model == 0 and (high.status == T.TRACKED).sum() == high.n_inliers[0]
    ref, cur, on_patch = _scene_a(1, "moving", 0.0)  # A: n_H = 255 < n_F = 300
    low, high = (T.ransac(ref, cur, status, T.IMAGE, 1.0, 512, 1, T.AUTO, p) for p in (0, 1000))
    assert low.model == 1 and high.model == 0 and high.n_inliers.tolist() == [300, 255]
    ref, cur, status, image = T.case("n5")  # no fundamental matrix: the homography at any p
    assert T.ransac(ref, cur, status, image, 1.0, 64, 1, T.AUTO, 1000).model == 1


def test_repeat_and_seed():
    ref, cur, _ = _scene_a(2, "moving", 0.3)
    a, b, c = (T.ransac(ref, cur, _all_tracked(300), T.IMAGE, 1.0, 64, seed, T.AUTO) for seed in (7, 7, 8))
    assert T.same_results(a, b) == [] and E.same(a.samples_h, b.samples_h) and E.same(a.samples_f, b.samples_f)
    assert not np.array_equal(a.samples_h, c.samples_h)


# ---- more than one camera motion: the pose family of tests/two_view_pose_ref.py -----------------------------------------

def test_the_pose_family_is_cleaned_as_far_as_its_scenes_determine_one_model():
    """The whole pose family.  Mode "fundamental" is tests/epipolar_ref.c's result bit for bit at every pose, so the bound that
    tests/test_epipolar_cpu.py asserts there holds here: no inlier rejected anywhere, no outlier kept where the scene determines one
    fundamental matrix, and the kept outliers of the three shallow scenes named there (KEPT_OUTLIERS) are these.  The homography on the plane
    (a pose per branch of TwoViewPose's quaternion, and forward motion) has check_scene_a's noise-free bound: every patch point rejected and
    no background point."""
    from tests import two_view_pose_ref as P
    from tests.test_epipolar_cpu import KEPT_OUTLIERS, family_filter_runs
    for pose, ref, cur, is_inlier, want, _ in family_filter_runs():
        r = T.ransac(ref, cur, _all_tracked(300), T.IMAGE, 1.0, 512, 1, "fundamental")
        assert r.model == 0 and E.same(r.status, want.status) and E.same(r.F, want.F) and E.same(r.counts[0], want.counts), pose
        assert int(((r.status == T.TRACKED) & ~is_inlier).sum()) == KEPT_OUTLIERS.get(pose, 0) and (r.status == T.TRACKED)[is_inlier].all(), pose
    for pose in P.FILTER_POSES:
        ref, cur, on_patch, _ = T.planar_scene(300, 1, "moving", 0.0, pose=P.family_pose(pose))
        r = T.ransac(ref, cur, _all_tracked(300), T.IMAGE, 1.0, 512, 1, "homography")
        rejected = r.status == T.LARGE_RESIDUAL
        assert int((rejected & on_patch).sum()) == int(on_patch.sum()) == 45 and not (rejected & ~on_patch).any(), pose
        assert r.model == 1 and r.n_inliers[1] == 255 == int((r.status == T.TRACKED).sum()), pose
