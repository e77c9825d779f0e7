"""The warm start of RAFT on video without a device: the scalar restatement (tests/flow_warm_ref.c) pinned by hand-built
known answers, against an independent float64 restatement in numpy (brute-force argmin) and against upstream RAFT's own route,
``scipy.interpolate.griddata(method="nearest")`` spelled as its ``forward_interpolate`` spells it; and three mutants each comparison that
can see them rejects.

Two choices of a source for one target are a *near-tie* when their float64 squared distances agree within NEAR_TIE relative.  Where the
bound comes from: the float32 rule rounds once in each of ex and ey, once in ex * ex and once in the fmaf, under 4 * 2^-24 relative on
d2 together; the bound is twice that.  Only at a near-tie may the restatement choose another source than float64, and at no more than
CAP of a case's pixels.  Measured on the cases below (printed by the tests, -s shows them): 0 differing pixels in every case against both."""
import functools

import numpy as np
import pytest

from tests import flow_warm_ref as R

NEAR_TIE = 8 * 2.0 ** -24
CAP = 0.01
NAN, INF = float("nan"), float("inf")
B = 2
# (name, H, W, sigma or None for whole-number flows in -3 .. 3)
CASES = [("8x8 sigma 2", 8, 8, 2.0), ("9x17 sigma 5", 9, 17, 5.0), ("33x65 sigma 8", 33, 65, 8.0), ("16x40 sigma 40", 16, 40, 40.0),
         ("12x20 integers", 12, 20, None)]
GAUSSIAN = [c for c in CASES if c[3] is not None]


def gaussian_flow(B, H, W, sigma, seed):
    return (np.random.default_rng(seed).standard_normal((B, 2, H, W)) * sigma).astype(np.float32)


def integer_flow(B, H, W, seed, reach=3):
    """Whole-number flows in -reach .. reach: landings coincide and targets sit at equal distances from several of them everywhere."""
    return np.random.default_rng(seed).integers(-reach, reach + 1, (B, 2, H, W)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(flow, the restatement's output, its chosen source per target) — computed once, shared, never written to."""
    _, H, W, sigma = next(c for c in CASES if c[0] == name)
    flow = integer_flow(B, H, W, 7) if sigma is None else gaussian_flow(B, H, W, sigma, 100 + H)
    out, chosen = R.warm(flow, with_chosen=True)
    for a in (flow, out, chosen):
        a.setflags(write=False)
    return flow, out, chosen


# ---- known answers -------------------------------------------------------------------------------------------------------------


def test_zero_flow():
    """Row 0 and column 0 land on x1 = 0 or y1 = 0, which the strict test refuses: their targets take the nearest source of the
    interior, target (0, 0) source (1, 1).  The flow is zero, so the values say nothing: the chosen indices do."""
    H, W = 4, 5
    out, chosen = R.warm(np.zeros((1, 2, H, W), np.float32), with_chosen=True)
    want = np.array([[max(y, 1) * W + max(x, 1) for x in range(W)] for y in range(H)])
    assert chosen[0].tolist() == want.tolist() and chosen[0, 0, 0] == 1 * W + 1
    assert out.view(np.uint32).max() == 0


def test_an_entry_without_a_valid_source_is_all_plus_zero():
    flow = np.full((2, 2, 3, 4), -100.0, np.float32)
    flow[1] = gaussian_flow(1, 3, 4, 0.3, 1)[0]
    out, chosen = R.warm(flow, with_chosen=True)
    assert (chosen[0] == -1).all() and out[0].view(np.uint32).max() == 0  # +0, not -0
    assert (chosen[1] >= 0).all()  # entries are independent
    assert R.same(out[1:], R.warm(flow[1:]))


@pytest.mark.parametrize("value", [NAN, INF, -INF, 1e30])
def test_a_non_finite_or_huge_flow_makes_only_its_source_invalid(value):
    H, W = 5, 6
    flow = np.full((1, 2, H, W), 0.25, np.float32)  # every source lands inside, a quarter pixel down and right of itself
    _, before = R.warm(flow, with_chosen=True)
    assert before[0].tolist() == np.arange(H * W).reshape(H, W).tolist()
    for channel in (0, 1):
        hurt = flow.copy()
        hurt[0, channel, 2, 3] = value
        out, chosen = R.warm(hurt, with_chosen=True)
        s = 2 * W + 3
        assert s not in chosen and np.isfinite(out).all()
        others = np.arange(H * W).reshape(H, W) != s
        assert (chosen[0][others] == before[0][others]).all()
        # its own target goes to a neighbour at one pixel's distance; the lowest index of them is the one above
        assert chosen[0, 2, 3] == 1 * W + 3


def test_two_sources_on_one_spot_the_lower_index_wins():
    H, W = 4, 6
    flow = np.full((1, 2, H, W), -100.0, np.float32)  # nothing else is valid
    flow[0, :, 1, 1] = (2.5, 1.5)    # source 7 lands on (3.5, 2.5)
    flow[0, :, 3, 4] = (-0.5, -0.5)  # source 22 lands on (3.5, 2.5) too, with another flow
    out, chosen = R.warm(flow, with_chosen=True)
    assert (chosen == 1 * W + 1).all() and (out[0, 0] == 2.5).all() and (out[0, 1] == 1.5).all()
    _, mutant = R.warm(flow, R.MUTANT_HIGHEST_INDEX, with_chosen=True)
    assert (mutant == 3 * W + 4).all()


def test_output_values_are_copies_of_the_input_floats():
    flow, out, chosen = case("9x17 sigma 5")
    Bn, _, H, W = flow.shape
    for b in range(Bn):
        for c in range(2):
            assert R.same(out[b, c], flow[b, c].reshape(-1)[chosen[b]])


# ---- against float64 -----------------------------------------------------------------------------------------------------------


def float64_landings(flow):
    """(x1, y1, valid) per batch entry in float64: the sum of a whole number and a float32 is exact there."""
    Bn, _, H, W = flow.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        x1, y1 = xs[None] + flow[:, 0].astype(np.float64), ys[None] + flow[:, 1].astype(np.float64)
        valid = (x1 > 0) & (x1 < W) & (y1 > 0) & (y1 < H)
    return x1.reshape(Bn, -1), y1.reshape(Bn, -1), valid.reshape(Bn, -1)


def float64_distances(flow):
    """d2[b][t][s] in float64, +inf at an invalid source."""
    Bn, _, H, W = flow.shape
    x1, y1, valid = float64_landings(flow)
    ty, tx = (a.reshape(-1).astype(np.float64) for a in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = (tx[None, :, None] - x1[:, None, :]) ** 2 + (ty[None, :, None] - y1[:, None, :]) ** 2
    return np.where(valid[:, None, :], d2, np.inf)


def float64_choice(flow):
    """The brute-force argmin (the first of equal minima: the lowest index) [B, H, W]."""
    Bn, _, H, W = flow.shape
    return float64_distances(flow).argmin(-1).reshape(Bn, H, W)


def compare_choices(flow, chosen, other):
    """(pixels where the two choices differ, those of them that are no near-tie), by the float64 distances of both choices."""
    Bn, _, H, W = flow.shape
    d2 = float64_distances(flow)
    mine = np.take_along_axis(d2, chosen.reshape(Bn, -1, 1).astype(np.int64), -1)[..., 0]
    theirs = np.take_along_axis(d2, other.reshape(Bn, -1, 1).astype(np.int64), -1)[..., 0]
    differ = chosen.reshape(Bn, -1) != other.reshape(Bn, -1)
    near = np.abs(mine - theirs) <= NEAR_TIE * np.maximum(mine, theirs)
    return int(differ.sum()), int((differ & ~near).sum())


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_restatement_against_float64(name):
    flow, _, chosen = case(name)
    differ, far = compare_choices(flow, chosen, float64_choice(flow))
    print(f"{name}: {differ} of {chosen.size} pixels choose another source than float64, {far} of them at no near-tie")
    assert far == 0
    assert differ <= CAP * chosen.size


# ---- against upstream's route ---------------------------------------------------------------------------------------------------


def forward_interpolate(flow):
    """Upstream RAFT's forward_interpolate (core/utils/utils.py) on one [2, H, W] array, as it is written there."""
    from scipy import interpolate

    dx, dy = flow[0], flow[1]
    ht, wd = dx.shape
    x0, y0 = np.meshgrid(np.arange(wd), np.arange(ht))
    x1 = x0 + dx
    y1 = y0 + dy
    x1 = x1.reshape(-1)
    y1 = y1.reshape(-1)
    dx = dx.reshape(-1)
    dy = dy.reshape(-1)
    valid = (x1 > 0) & (x1 < wd) & (y1 > 0) & (y1 < ht)
    x1 = x1[valid]
    y1 = y1[valid]
    dx = dx[valid]
    dy = dy[valid]
    flow_x = interpolate.griddata((x1, y1), dx, (x0, y0), method="nearest", fill_value=0)
    flow_y = interpolate.griddata((x1, y1), dy, (x0, y0), method="nearest", fill_value=0)
    return np.stack([flow_x, flow_y], axis=0).astype(np.float32)


def upstream_choice(flow):
    """The source upstream's route takes per target [B, H, W]: griddata returns values, so it is asked for the sources' own indices."""
    from scipy import interpolate

    Bn, _, H, W = flow.shape
    x1, y1, valid = float64_landings(flow)
    x0, y0 = np.meshgrid(np.arange(W), np.arange(H))
    out = np.empty((Bn, H, W), np.int64)
    for b in range(Bn):
        index = np.flatnonzero(valid[b])
        out[b] = interpolate.griddata((x1[b][index], y1[b][index]), index.astype(np.float64), (x0, y0), method="nearest", fill_value=0)
    return out


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_restatement_against_scipy_griddata(name):
    """The same near-tie rule.  On the Gaussian flows nothing may differ, neither a choice nor a value of forward_interpolate itself.  On
    the whole-number flows equal distances are everywhere and upstream's k-d tree returns whichever of them it meets first, where the
    contract takes the lowest index: there every difference must be a tie, and their number is upstream's, not ours to bound."""
    pytest.importorskip("scipy")
    flow, out, chosen = case(name)
    differ, far = compare_choices(flow, chosen, upstream_choice(flow))
    print(f"{name}: {differ} of {chosen.size} pixels choose another source than griddata(nearest), {far} of them at no near-tie")
    assert far == 0
    if name in [c[0] for c in GAUSSIAN]:
        assert differ == 0
        for b in range(flow.shape[0]):
            assert R.same(out[b], forward_interpolate(flow[b]))


# ---- the mutants ---------------------------------------------------------------------------------------------------------------


def test_mutant_highest_index_fails_where_ties_are():
    """Against float64 on the whole-number flows: a tie is a near-tie, so the mutant is caught by the values it copies and by the cap."""
    flow, out, chosen = case("12x20 integers")
    mutant_out, mutant = R.warm(flow, R.MUTANT_HIGHEST_INDEX, with_chosen=True)
    differ, far = compare_choices(flow, mutant, float64_choice(flow))
    print(f"highest index wins: {differ} of {mutant.size} pixels differ from float64 ({far} at no near-tie)")
    assert compare_choices(flow, chosen, float64_choice(flow)) == (0, 0)
    assert far == 0 and differ > CAP * mutant.size
    assert not R.same(mutant_out, out)


def test_mutant_closed_bounds_fails_the_known_answer_and_float64():
    _, chosen = R.warm(np.zeros((1, 2, 4, 5), np.float32), R.MUTANT_CLOSED_BOUNDS, with_chosen=True)
    assert chosen[0, 0, 0] == 0  # the contract: 6
    flow = integer_flow(B, 12, 20, 7)  # whole-number landings on x1 = 0, y1 = 0, x1 = W, y1 = H are what the mutant admits
    _, mutant = R.warm(flow, R.MUTANT_CLOSED_BOUNDS, with_chosen=True)
    differ, far = compare_choices_allowing_invalid(flow, mutant)
    print(f"closed bounds: {differ} pixels differ from float64, {far} at no near-tie")
    assert far > 0


def compare_choices_allowing_invalid(flow, chosen):
    """compare_choices against float64 where ``chosen`` may name a source float64 holds invalid (distance +inf: never a near-tie)."""
    Bn = flow.shape[0]
    d2 = float64_distances(flow)
    mine = np.take_along_axis(d2, chosen.reshape(Bn, -1, 1).astype(np.int64), -1)[..., 0]
    best = d2.min(-1)
    differ = chosen.reshape(Bn, -1) != d2.argmin(-1)
    with np.errstate(invalid="ignore"):
        near = np.isfinite(mine) & (np.abs(mine - best) <= NEAR_TIE * np.maximum(mine, best))
    return int(differ.sum()), int((differ & ~near).sum())


@pytest.mark.parametrize("name", [c[0] for c in GAUSSIAN])
def test_mutant_swapped_xy_fails_float64(name):
    flow, _, _ = case(name)
    _, mutant = R.warm(flow, R.MUTANT_SWAPPED_XY, with_chosen=True)
    differ, far = compare_choices(flow, mutant, float64_choice(flow))
    print(f"{name}, ex and ey swapped: {differ} of {mutant.size} pixels differ from float64, {far} at no near-tie")
    assert far > 0 and differ > CAP * mutant.size
