"""The restatement of the keypoint decoder (tests/keypoint_decode_ref.c) pinned without a device: known answers by hand,
an independent numpy float64 composition on the shapes the GPU tests use, five mutants each caught by one of those, the selection
invariants on random occupied sets, and what the oracle's matcher makes of the zero rows behind ``count``."""
import numpy as np
import pytest

from tests import keypoint_decode_ref as R

# Measured over CASES (printed by test_restatement_against_float64): the worst |score - float64| is 3.9e-7 (scores up to 0.9 whose
# numerator and denominator both carry exp_c's 2 ulp) and the worst |descriptor entry - float64| 5.5e-8 (entries of a unit vector: the
# blend's roundings, the norm's and the division's).  Asserted at 4 x the measured values, as DESIGN.md 5.20 does.
SCORE_TOL = 4 * 3.9e-7
DESC_TOL = 4 * 5.5e-8
TIE_CAP = 0.02  # selected pixels may differ from float64's only at near-ties, and in at most 2 % of the keypoints


def compare_with_float64(semi, desc, K, kw, variant=R.CONTRACT):
    """(worst score deviation, worst descriptor deviation, rows that differ from float64's, rows, differing rows no near-tie explains)."""
    got = R.decode(semi, desc, max_keypoints=K, variant=variant, **kw)
    pixels, heat, descriptor_of = R.decode_float64(semi, desc, K, kw["min_score"], kw["min_distance"], kw["border"], kw.get("occupied"), kw.get("occupied_mask"))
    H, W = heat.shape
    score_dev = float(np.abs(got.heatmap.astype(np.float64) - heat).max())
    mine = (got.uv[:got.count, 1].astype(np.int64) * W + got.uv[:got.count, 0].astype(np.int64))
    assert R.same(got.scores[:got.count], got.heatmap.reshape(-1)[mine])
    desc_dev = 0.0
    for r, pixel in enumerate(mine):
        desc_dev = max(desc_dev, float(np.abs(got.descriptors[r].astype(np.float64) - descriptor_of(pixel)).max()))
    rows = max(len(mine), len(pixels))
    differing = [r for r in range(rows) if r >= len(mine) or r >= len(pixels) or mine[r] != pixels[r]]
    reach = max(kw["min_distance"], 1) - 1
    flat = heat.reshape(-1)
    unexplained = 0
    for r in differing:
        for pixel in ([mine[r]] if r < len(mine) else []) + ([pixels[r]] if r < len(pixels) else []):
            y, x = divmod(int(pixel), W)
            s = flat[pixel]
            win = heat[max(y - reach, 0):y + reach + 1, max(x - reach, 0):x + reach + 1]
            near = np.abs(win - s)
            # a near-tie: another score of the window within the tolerance but not equal (an exact tie is decided by the stated rule), or
            # the score within the tolerance of min_score
            if not (((near <= SCORE_TOL) & (near > 0)).any() or abs(s - kw["min_score"]) <= SCORE_TOL):
                unexplained += 1
    return score_dev, desc_dev, len(differing), rows, unexplained


def test_one_cell_of_equal_logits_scores_one_65th():
    semi = np.full((65, 1, 1), 0.75, np.float32)
    got = R.decode(semi, np.ones((4, 1, 1), np.float32), max_keypoints=4, min_score=0.0, min_distance=1, border=0)
    assert (got.heatmap == np.float32(1.0) / np.float32(65.0)).all()
    # 64 equal scores, distance 1: every pixel survives, the lower pixel index first
    assert got.survivors == 64 and got.count == 4 and got.uv.tolist() == [[0, 0], [1, 0], [2, 0], [3, 0]]
    assert (got.descriptors == np.float32(0.5)).all()  # (1, 1, 1, 1) / 2


def test_one_dominant_logit_gives_one_keypoint_at_its_pixel():
    semi = np.zeros((65, 2, 2), np.float32)
    semi[19, 1, 0] = 20.0  # cell (1, 0), k = 19: row 8 + 19 / 8 = 10, column 0 + 19 % 8 = 3
    desc = np.zeros((3, 2, 2), np.float32)
    desc[:, 0, 0], desc[:, 1, 0] = (3.0, 0.0, 4.0), (0.0, 5.0, 0.0)
    got = R.decode(semi, desc, max_keypoints=5, min_score=0.1, min_distance=20, border=0)
    assert got.count == 1 and got.uv[0].tolist() == [3.0, 10.0] and got.scores[0] > 0.99
    assert (got.uv[1:] == 0).all() and (got.scores[1:] == 0).all() and (got.descriptors[1:] == 0).all()
    # xc = max((3 - 3.5) / 8, 0) = 0, yc = (10 - 3.5) / 8 = 0.8125: 0.1875 (3, 0, 4) + 0.8125 (0, 5, 0), normalised
    v = np.float32([0.1875 * 3, 0.8125 * 5, 0.1875 * 4])
    assert np.abs(got.descriptors[0] - v / np.linalg.norm(v)).max() < 1e-6


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_the_two_descriptor_layouts_give_the_same_bits(layout):
    semi, desc, kw = R.case("tile_rows_d4_occupied")
    assert R.same_results(R.decode(semi, desc, max_keypoints=50, layout=layout, **kw), R.decode(semi, desc, max_keypoints=50, **kw)) == []


def test_restatement_against_float64():
    worst_score = worst_desc = 0.0
    keypoints = differing = 0
    for name in R.CASES:
        semi, desc, kw = R.case(name)
        full = R.decode(semi, desc, max_keypoints=4096, **kw)
        assert 0 < full.survivors < 4096, name
        for K in sorted({max(full.survivors // 2, 1), 4096}):
            score_dev, desc_dev, n_diff, rows, unexplained = compare_with_float64(semi, desc, K, kw)
            print(f"{name} K={K}: S={full.survivors} rows={rows} score dev {score_dev:.3g} descriptor dev {desc_dev:.3g} differing {n_diff}")
            assert unexplained == 0, (name, K)
            worst_score, worst_desc = max(worst_score, score_dev), max(worst_desc, desc_dev)
            keypoints, differing = keypoints + rows, differing + n_diff
    print(f"worst score deviation {worst_score:.3g}, worst descriptor deviation {worst_desc:.3g}, {differing} of {keypoints} rows differ")
    assert worst_score <= SCORE_TOL and worst_desc <= DESC_TOL
    assert differing <= TIE_CAP * keypoints  # the seeds of CASES stay within the cap


def test_exact_ties_follow_the_stated_rule_in_float64_too():
    semi, desc = R.tie_heads()
    kw = dict(min_score=0.05, min_distance=9, border=0)
    got = R.decode(semi, desc, max_keypoints=64, **kw)
    _, _, n_diff, rows, _ = compare_with_float64(semi, desc, 64, kw)
    assert n_diff == 0 and rows == got.count
    # the strongest pixel of cell (0, 0) survives, its twin in cell (0, 1) is suppressed, the twin in cell (2, 4) follows it directly
    uv = got.uv[:got.count]
    twin = [r for r in range(got.count - 1) if got.scores[r] == got.scores[r + 1]]
    assert len(twin) == 1
    a, b = uv[twin[0]], uv[twin[0] + 1]
    assert (b - a).tolist() == [32.0, 16.0] and a[0] < 8 and a[1] < 8
    assert not any((u == a + np.float32([8.0, 0.0])).all() for u in uv)


def _caught_by_float64(variant, semi, desc, K, kw):
    score_dev, desc_dev, n_diff, rows, unexplained = compare_with_float64(semi, desc, K, kw, variant)
    return score_dev > SCORE_TOL or desc_dev > DESC_TOL or unexplained > 0 or n_diff > TIE_CAP * rows


def test_each_mutant_is_caught():
    semi, desc, kw = R.case("tile_rows_d4_occupied")
    assert not _caught_by_float64(R.CONTRACT, semi, desc, 4096, kw)
    # the dustbin left out of the denominator: the known answer 1 / 65 becomes 1 / 64
    equal = np.full((65, 1, 1), 0.75, np.float32)
    flat = dict(max_keypoints=4, min_score=0.0, min_distance=1, border=0)
    assert (R.decode(equal, np.ones((4, 1, 1), np.float32), variant=R.MUTANTS["dustbin_left_out_of_the_denominator"], **flat).heatmap == np.float32(1.0) / np.float32(64.0)).all()
    assert _caught_by_float64(R.MUTANTS["dustbin_left_out_of_the_denominator"], semi, desc, 4096, kw)
    # k / 8 and k % 8 exchanged: the dominant logit's keypoint lands at the transposed pixel of its cell
    one = np.zeros((65, 2, 2), np.float32)
    one[19, 1, 0] = 20.0
    got = R.decode(one, np.ones((3, 2, 2), np.float32), max_keypoints=5, min_score=0.1, min_distance=20, border=0, variant=R.MUTANTS["k_div_8_and_k_mod_8_exchanged"])
    assert got.count == 1 and got.uv[0].tolist() == [2.0, 11.0]
    assert _caught_by_float64(R.MUTANTS["k_div_8_and_k_mod_8_exchanged"], semi, desc, 4096, kw)
    # the sample without the cell-centre shift, and the normalisation per corner: the descriptors leave float64's
    for name in ("no_cell_centre_shift", "normalised_per_corner_before_blending"):
        _, desc_dev, n_diff, _, _ = compare_with_float64(semi, desc, 4096, kw, R.MUTANTS[name])
        assert n_diff == 0 and desc_dev > 100 * DESC_TOL, name
    # the higher pixel index first on a tie: the exact ties of tie_heads come out the other way round
    tie_semi, tie_desc = R.tie_heads()
    tie_kw = dict(min_score=0.05, min_distance=9, border=0)
    assert not _caught_by_float64(R.CONTRACT, tie_semi, tie_desc, 64, tie_kw)
    assert _caught_by_float64(R.MUTANTS["higher_pixel_index_first_on_a_tie"], tie_semi, tie_desc, 64, tie_kw)


@pytest.mark.parametrize("seed", range(4))
def test_selection_invariants_on_random_occupied_sets(seed):
    rng = np.random.default_rng(300 + seed)
    hc, wc = 5, 9
    semi, desc = R.heads(hc, wc, 8, 400 + seed)
    d, border = int(rng.integers(2, 12)), int(rng.integers(0, 7))
    occupied, mask = R.occupied_points(hc, wc, 25, 500 + seed)
    got = R.decode(semi, desc, max_keypoints=2048, min_score=0.03, min_distance=d, border=border, occupied=occupied, occupied_mask=mask)
    H, W = 8 * hc, 8 * wc
    uv = got.uv[:got.count].astype(np.int64)
    assert got.count == got.survivors and got.count >= 1
    cheb = np.abs(uv[:, None, :] - uv[None, :, :]).max(axis=2) + d * np.eye(len(uv), dtype=np.int64)
    assert cheb.min() >= d  # pairwise Chebyshev distance >= d
    stamps = np.stack([np.clip(np.floor(occupied[:, 0] + np.float32(0.5)), 0, W - 1), np.clip(np.floor(occupied[:, 1] + np.float32(0.5)), 0, H - 1)], axis=1)
    stamps = stamps[mask != 0].astype(np.int64)
    assert np.abs(uv[:, None, :] - stamps[None, :, :]).max(axis=2).min() > d - 1  # none within reach of a stamp
    assert (uv[:, 0] >= border).all() and (uv[:, 0] < W - border).all() and (uv[:, 1] >= border).all() and (uv[:, 1] < H - border).all()
    assert (np.diff(got.scores[:got.count]) <= 0).all() and (got.scores[:got.count] > 0.03).all()
    # a masked-out point blocks nobody: without the mask there are no more survivors than with it
    assert R.decode(semi, desc, max_keypoints=2048, min_score=0.03, min_distance=d, border=border, occupied=occupied).survivors <= got.survivors


def test_hostile_heads_propagate_and_do_not_stop_the_restatement():
    semi, desc = R.hostile_heads()
    got = R.decode(semi, desc, max_keypoints=512, min_score=0.01, min_distance=1, border=0)
    assert np.isnan(got.heatmap[0:8, 0:16]).all() and np.isnan(got.heatmap[8:16, 8:16]).all()  # a NaN logit, and the cell of all -inf
    assert (got.heatmap[8:16, 16:24] == 0).all()  # the dustbin took everything
    assert got.count > 50 and not np.isnan(got.scores).any() and np.isnan(got.descriptors).any()


def test_the_oracle_matcher_gives_a_zero_descriptor_no_match():
    """A zero row's cosine distance is 0.5 - (0 / 0) / |b| * 0.5 = NaN, which is below no threshold: the rows behind ``count`` neither find a
    partner nor are found, whatever the threshold (README, the KeypointDecoder section)."""
    from tests import oracle_lib
    rng = np.random.default_rng(5)
    a = rng.standard_normal((6, 16)).astype(np.float32)
    a[4:] = 0
    b = np.vstack([a[:4][::-1], np.zeros((2, 16), np.float32)])
    ok, idx = oracle_lib.match_float(a, b, 1.0)
    assert ok and idx.tolist() == [3, 2, 1, 0, -1, -1]
