"""The oracle against ref64 (tests/klt_ref64.py), a float64 restatement of the reference's KLT family written independently of
oracle/*.c, at the north-star bar (1e-3 px per feature, BASELINE.json); the kernels directly in tests/test_klt_ref64_gpu.py.

Which features are compared is decided by ref64's own report, never by the result under test:
* one step (kMaxIteration 1; the single-level overload, and for LSSD, whose single-level overload never writes its result back,
  also a one-level pyramid): not singular, at least one valid pixel, conditioning at most ONE_STEP_COND, the convergence and
  outside decisions outside the band;
* full tracking (pyramid overload): every decision margin outside the band (relative BAND_REL of each threshold, BAND_PX px from
  the outside bounds, BAND_EDGE_PX from validity edges), conditioning at most FULL_COND; statuses and iteration counts equal,
  kTracked positions within 1e-3 px except where a level ran out of iterations (no fixed point: the position is not compared).
  At most MAX_BAND of a variant's features may lie in the band.

Conditioning is Skeel's number of the new position (klt_ref64._solve): to first order, float32 rounding of the sums moves the
position by about 6e-8 x cond px.  The filters are narrower than 1e4 where the measured spread needed it: the affine and LSSD normal
equations use absolute image coordinates (affine_klt.cpp:157-158, lssd_klt.cpp:210), so a float32 implementation's spread grows
with the distance from the image origin; at 1e4 it reached 2e-3 px (affine, one step) and 5e-3 px (LSSD).  The edge band is 1e-4
px, not 1e-3: with 1e-3 a feature whose patch straddles an image edge almost always has one of its ~10 000 samples inside it, and
5 % of the affine features fell in the band for that alone.
"""
import functools
import os

import numpy as np
import pytest

from feature_tracker_amd import synth
from tests import klt_ref64 as R64
from tests import scenes

TOL_PX = 1e-3       # per feature (north star)
P99_PX = 1e-4       # 99th percentile of the one-step comparison
# conditioning filters, narrowed from 1e4 to what the measured float32-vs-float64 spread needs (module docstring)
ONE_STEP_COND = {"basic": 1e3, "affine": 3e2, "lssd": 1e2}
FULL_COND = {"basic": 3e2, "affine": 1e2, "lssd": 3e1}
BAND_REL, BAND_PX, BAND_EDGE_PX = 1e-3, 1e-3, 1e-4
MAX_BAND = 0.02

MODELS = ["basic", "affine", "lssd"]
METHODS = ["inverse", "direct", "fast"]
# consider_patch_luminance only changes the fast LSSD variant (lssd_klt_fast.cpp:27,65); the non-fast ones always mean-normalise
VARIANTS = [(m, k, False) for m in MODELS for k in METHODS] + [("lssd", "fast", True)]
VARIANT_IDS = [f"{m}-{k}" + ("-luminance" if lum else "") for m, k, lum in VARIANTS]
HALVES = [(1, 1), (2, 2), (6, 6), (7, 7), (15, 15), (3, 9)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def example_pair(levels=4):
    """The reference's example pair (tests/data/optical_flow) with the truncating pyramid."""
    from PIL import Image
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "optical_flow")
    ref = np.array(Image.open(os.path.join(root, "ref_image.png")).convert("L"), dtype=np.uint8)
    cur = np.array(Image.open(os.path.join(root, "cur_image.png")).convert("L"), dtype=np.uint8)
    return tuple(synth.build_pyramid(ref, levels)), tuple(synth.build_pyramid(cur, levels))


@functools.lru_cache(maxsize=None)
def small_pair():
    """Small coordinates keep the affine / LSSD normal equations well conditioned right up to the far image edges."""
    ref, cur = synth.make_image_pair(64, 48, (1.3, -0.8), rotation_deg=1.0, scale=1.01)
    return (ref,), (cur,)


@functools.lru_cache(maxsize=None)
def odd_pair():
    ref, cur = synth.make_image_pair(333, 251, (2.6, 1.7), rotation_deg=1.0, scale=1.01)
    return (ref,), (cur,)


def one_step_inputs():
    return {
        "example": example_pair(1),
        "translation-easy": scenes.scene(320, 240, 1, "easy", "translation"),
        "translation-hard": scenes.scene(320, 240, 1, "hard", "translation"),
        "similarity-easy": scenes.scene(320, 240, 1, "easy", "similarity"),
        "similarity-hard": scenes.scene(320, 240, 1, "hard", "similarity"),
        "odd-333x251": odd_pair(),
        "small-64x48": small_pair(),
    }


def harris(oracle, image, n, min_distance, min_response):
    return oracle.harris_detect(image, n, min_distance, min_response)


def feature_sets(oracle, image, hr, hc, seed=0):
    """Harris corners, random positions, a band within half + 2 px of every edge (partly valid patches) and sub-pixel positions
    that put patch samples exactly on lattice / validity edges (integers, .5, rows - 1 - half, ...)."""
    rows, cols = image.shape
    rs = np.random.RandomState(seed)
    corners = harris(oracle, image, 80, 8, 10.0)
    rand = np.stack([rs.uniform(0, cols - 1, 80), rs.uniform(0, rows - 1, 80)], 1)
    m = max(hr, hc) + 2
    side = rs.randint(0, 4, 120)
    band = np.stack([rs.uniform(0, cols - 1, 120), rs.uniform(0, rows - 1, 120)], 1)
    band[side == 0, 0] = rs.uniform(-1, m, (side == 0).sum())
    band[side == 1, 0] = cols - 1 - rs.uniform(-1, m, (side == 1).sum())
    band[side == 2, 1] = rs.uniform(-1, m, (side == 2).sum())
    band[side == 3, 1] = rs.uniform(-1, m, (side == 3).sum())
    xs = [0.0, 1.0, hc - 1.0, float(hc), hc + 1.0, hc + 0.5, cols - 1.0, cols - 3.0 - hc, cols - 2.0 - hc, cols - 1.0 - hc, cols - 2.5 - hc, cols / 2 + 0.5]
    ys = [0.0, 1.0, hr - 1.0, float(hr), hr + 1.0, hr + 0.5, rows - 1.0, rows - 3.0 - hr, rows - 2.0 - hr, rows - 1.0 - hr, rows - 2.5 - hr, rows / 2 + 0.5]
    edge = np.array([(x, y) for x in xs for y in ys])
    return np.concatenate([corners, rand, band, edge]).astype(np.float32)


# ---- criteria -------------------------------------------------------------------------------------------------------------------

def one_step_check(model, ref, uv, status, what, cond_max=None):
    """Returns (ok, message, failure factor, stats).  uv / status: the implementation under test."""
    uv = np.asarray(uv, np.float64)
    cond_max = ONE_STEP_COND[model] if cond_max is None else cond_max
    sel = ref.comparable(cond_max) & ref.away(BAND_REL, BAND_PX, BAND_EDGE_PX)
    d = np.abs(uv - ref.uv).max(axis=1)
    fin = np.isfinite(ref.uv).all(axis=1)
    dsel = d[sel & fin]
    st_bad = int(np.count_nonzero(status[sel] != ref.status[sel]))
    mx = float(dsel.max()) if dsel.size else 0.0
    p99 = float(np.percentile(dsel, 99)) if dsel.size else 0.0
    nan_bad = int(np.count_nonzero(np.isfinite(uv[sel]).all(axis=1) != fin[sel]))
    factor = max(mx / TOL_PX, p99 / P99_PX, st_bad + nan_bad)
    stats = dict(n=len(uv), compared=int(sel.sum()), singular=int(ref.singular.sum()),
                 ill_conditioned=int(((ref.cond > cond_max) & ~ref.singular).sum()),
                 in_band=int((~ref.away(BAND_REL, BAND_PX, BAND_EDGE_PX)).sum()), max=mx, p99=p99, status_mismatch=st_bad)
    ok = mx <= TOL_PX and p99 <= P99_PX and st_bad == 0 and nan_bad == 0
    return ok, f"{what}: {stats}", factor, stats


def full_check(model, ref, uv, status, iters, what, cond_max=None):
    uv = np.asarray(uv, np.float64)
    cond_max = FULL_COND[model] if cond_max is None else cond_max
    inside = ~ref.away(BAND_REL, BAND_PX, BAND_EDGE_PX)
    band = inside.mean()
    # a level that ran out of iterations leaves a position that is no fixed point: its status and iteration count are decided,
    # its position is not compared
    decided = ~inside & ~ref.singular & (ref.cond <= cond_max)
    away = decided & ~ref.capped
    st_bad = int(np.count_nonzero(status[decided] != ref.status[decided]))
    it_bad = int(np.count_nonzero(iters[decided] != ref.iters[decided])) if iters is not None else 0
    tr = away & (ref.status == R64.TRACKED) & (status == R64.TRACKED)
    d = np.abs(uv[tr] - ref.uv[tr]).max(axis=1) if tr.any() else np.zeros(1)
    mx = float(d.max())
    factor = max(mx / TOL_PX, band / MAX_BAND, st_bad, it_bad)
    stats = dict(n=len(uv), compared=int(away.sum()), in_band=int(inside.sum()), capped=int(ref.capped.sum()),
                 ill_conditioned=int((ref.cond > cond_max).sum()),
                 singular=int(ref.singular.sum()), tracked=int(tr.sum()), band_fraction=round(float(band), 4), max=mx,
                 p99=float(np.percentile(d, 99)), status_mismatch=st_bad, iteration_mismatch=it_bad)
    ok = mx <= TOL_PX and st_bad == 0 and it_bad == 0  # the band fraction is asserted over all cases of a variant
    return ok, f"{what}: {stats}", factor, stats


# ---- the cases, shared with the GPU file ----------------------------------------------------------------------------------------

def one_step_cases(oracle):
    """(name, ref image, cur image, ref uv, cur uv, status, options): every half on the example pair, half 6 and the rectangular
    patch on the synthetic and odd-sized pairs; one case with a prediction, incoming failures and a kMaxTrackPointsNumber cap."""
    out = []
    for name, (rl, cl) in one_step_inputs().items():
        halves = HALVES if name == "example" else [(6, 6), (3, 9)]
        for hr, hc in halves:
            uv = feature_sets(oracle, rl[0], hr, hc, seed=hr * 31 + hc)
            out.append((f"{name}/{hr}x{hc}", rl[0], cl[0], uv, None, None, dict(half=hr, half_cols=hc)))
    rl, cl = scenes.scene(320, 240, 1, "hard", "similarity")
    uv = feature_sets(oracle, rl[0], 6, 6, seed=5)
    rs = np.random.RandomState(9)
    pred = (uv + np.float32([11.0, -8.0]) + rs.uniform(-1, 1, uv.shape)).astype(np.float32)
    status = (np.arange(len(uv)) % 7 == 3).astype(np.uint8) * (2 + (np.arange(len(uv)) % 3)).astype(np.uint8)
    out.append(("similarity-hard/prediction+status+cap", rl[0], cl[0], uv, pred, status, dict(half=6, max_points=len(uv) - 17)))
    # an exact two-pixel prediction: current-image samples land exactly on the far validity edges while the reference patch's
    # own lattice (and its gradient) is still valid there
    rl, cl = small_pair()
    uv = feature_sets(oracle, rl[0], 6, 6, seed=8)
    out.append(("small-64x48/edge prediction", rl[0], cl[0], uv, uv + np.float32([2.0, 2.0]), None, dict(half=6)))
    return out


def full_cases(oracle):
    """(name, ref levels, cur levels, ref uv, cur uv, status, options)."""
    rl, cl = example_pair(4)
    hard_t = scenes.scene(320, 240, 4, "hard", "translation")
    hard_s = scenes.scene(320, 240, 4, "hard", "similarity")
    uv_s = scenes.features(300, 320, 240, half=6, seed=99)
    small_s = scenes.scene(160, 120, 3, "hard", "similarity")
    uv_small = scenes.features(300, 160, 120, half=6, seed=99)
    return [
        ("example/300 Harris", rl, cl, harris(oracle, rl[0], 300, 25, 40.0), None, None, {}),
        ("example/2000 Harris", rl, cl, harris(oracle, rl[0], 2000, 4, 0.5), None, None, {}),
        ("translation-hard", hard_t[0], hard_t[1], uv_s, None, None, {}),
        ("similarity-hard", hard_s[0], hard_s[1], uv_s, None, None, {}),
        ("similarity-hard/rect, options, prediction, status", hard_s[0], hard_s[1], uv_s, uv_s + np.float32([9.0, -6.0]),
         (np.arange(300) % 9 == 4).astype(np.uint8) * 3,
         dict(half=3, half_cols=7, max_iteration=8, max_large_step=2, converge=1e-2, max_points=280)),
        # two iterations a level, one large step tolerated: features reach kTracked at a coarse level and stop on the large-step
        # test or the iteration cap at a finer one, so statuses carried across levels differ from statuses reset per level
        ("similarity-hard/2 iterations", hard_s[0], hard_s[1], uv_s, None, None, dict(max_iteration=2, max_large_step=1)),
        ("small-160x120/2 iterations", small_s[0], small_s[1], uv_small, None, None, dict(max_iteration=2, max_large_step=1)),
    ]


PRIOR = np.float32([[1.02, -0.026], [0.026, 1.02]])


def _kw(opt):
    return dict(dict(max_points=100000), **opt)


def run_ref(kind, model, method, lum, case, flags=R64.DEFAULT, prior=None):
    """kind: "one" (single-level overload, one iteration), "one-pyr" (a one-level pyramid, one iteration: the overload that writes
    LSSD's result back), "full" (pyramid overload)."""
    name, ri, ci, uv, cur, st, opt = case
    if kind == "one":
        return R64.track_single(model, method, ri, ci, uv, cur, st, max_iteration=1, prior=prior, luminance=lum, flags=flags, **_kw(opt))
    if kind == "one-pyr":
        return R64.track_pyramid(model, method, [ri], [ci], uv, cur, st, max_iteration=1, prior=prior, luminance=lum, flags=flags, **_kw(opt))
    return R64.track_pyramid(model, method, ri, ci, uv, cur, st, prior=prior, luminance=lum, flags=flags, **_kw(opt))


def run_oracle(oracle, kind, model, method, lum, case, prior=None):
    name, ri, ci, uv, cur, st, opt = case
    kw = dict(prior=prior, consider_luminance=lum, method=method, **_kw(opt))
    if kind == "one":
        _, c, s, it = oracle.klt_track_single(model, ri, ci, uv, cur, st, max_iteration=1, **kw)
    elif kind == "one-pyr":
        _, c, s, it = oracle.klt_track_pyramid(model, [ri], [ci], uv, cur, st, max_iteration=1, **kw)
    else:
        _, c, s, it = oracle.klt_track_pyramid(model, ri, ci, uv, cur, st, **kw)
    return c, s, it


def one_kinds(model):
    return ["one", "one-pyr"] if model == "lssd" else ["one"]


@functools.lru_cache(maxsize=None)
def _cases(kind):
    from tests import oracle_lib
    oracle_lib.lib()
    return one_step_cases(oracle_lib) if kind.startswith("one") else full_cases(oracle_lib)


def check_one_step_variant(run_impl, model, method, lum):
    """Every one-step case through `run_impl(kind, model, method, lum, case, prior)` -> (uv, status, iters); the prior on the
    prediction case only.  Returns the aggregate report."""
    agg = {}
    for kind in one_kinds(model):
        for case in _cases(kind):
            for prior in ([None, PRIOR] if model != "basic" and "prediction" in case[0] else [None]):
                ref = run_ref(kind, model, method, lum, case, prior=prior)
                c, s, _ = run_impl(kind, model, method, lum, case, prior)
                ok, msg, _, stats = one_step_check(model, ref, c, s, f"{model}/{method} {kind} {case[0]} prior={prior is not None}")
                assert ok, msg
                for k in ("max", "p99"):
                    agg[k] = max(agg.get(k, 0.0), stats[k])
                for k in ("n", "compared", "singular", "ill_conditioned", "in_band"):
                    agg[k] = agg.get(k, 0) + stats[k]
    return agg


def check_full_variant(run_impl, model, method, lum):
    agg = {}
    for case in _cases("full"):
        for prior in ([None, PRIOR] if model != "basic" and "prediction" in case[0] else [None]):
            ref = run_ref("full", model, method, lum, case, prior=prior)
            c, s, it = run_impl("full", model, method, lum, case, prior)
            ok, msg, _, stats = full_check(model, ref, c, s, it, f"{model}/{method} {case[0]} prior={prior is not None}")
            assert ok, msg
            agg["max"] = max(agg.get("max", 0.0), stats["max"])
            agg["p99"] = max(agg.get("p99", 0.0), stats["p99"])
            for k in ("n", "compared", "tracked", "in_band", "capped", "ill_conditioned", "singular"):
                agg[k] = agg.get(k, 0) + stats[k]
    band = agg["in_band"] / agg["n"]
    assert band <= MAX_BAND, f"{model}/{method}: {band:.3%} of the features lie in the decision band ({agg})"
    agg["band_fraction"] = round(band, 4)
    return agg


def _oracle_runner(oracle):
    return lambda kind, model, method, lum, case, prior: run_oracle(oracle, kind, model, method, lum, case, prior)


# ---- 1. one step ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model,method,lum", VARIANTS, ids=VARIANT_IDS)
def test_one_step_oracle_matches_ref64(oracle, model, method, lum):
    agg = check_one_step_variant(_oracle_runner(oracle), model, method, lum)
    print(f"\nONE-STEP oracle {model}/{method}{' luminance' if lum else ''}: {agg}")


# ---- 2. full tracking -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model,method,lum", VARIANTS, ids=VARIANT_IDS)
def test_full_tracking_oracle_matches_ref64(oracle, model, method, lum):
    agg = check_full_variant(_oracle_runner(oracle), model, method, lum)
    print(f"\nFULL oracle {model}/{method}{' luminance' if lum else ''}: {agg}")


# ---- 3. known answers, derived by hand (the same ones tests/test_oracle_cpu.py holds the oracle to) -----------------------------

def _ramp_pair(shift):
    x = np.arange(128, dtype=np.int32)
    ref = np.tile(np.clip(2 * x, 0, 255).astype(np.uint8), (64, 1))
    cur = np.tile(np.clip(2 * (x - shift), 0, 255).astype(np.uint8), (64, 1))
    return ref, cur


def test_half_length_step_sequence_on_I_equals_2x():
    """I = 2x shifted by 2 px: without the 1/2 of the central difference fx = 4, ft = -4, so the first step is 1 px (fy = 0: H is
    singular, v_y = 0); then 0.5, 0.25, 0.125 (0.125^2 < 4e-2): kTracked after 4 iterations at 61.875."""
    ref, cur = _ramp_pair(2)
    uv = np.float32([[60.0, 30.0]])
    for method in ("inverse", "direct", "fast"):
        r = R64.track_single("basic", method, ref, cur, uv, half=3, max_iteration=1)
        assert r.uv.tolist() == [[61.0, 30.0]] and r.iters.tolist() == [1] and r.singular[0], method
        assert r.status.tolist() == ([R64.LARGE_RESIDUAL] if method == "fast" else [R64.NOT_TRACKED]), method
    r = R64.track_single("basic", "inverse", ref, cur, uv, half=3)
    assert r.uv.tolist() == [[61.875, 30.0]] and r.status.tolist() == [R64.TRACKED] and r.iters.tolist() == [4]
    # with the 1/2 restored Gauss-Newton lands in one step
    r = R64.track_single("basic", "inverse", ref, cur, uv, half=3, max_iteration=1, flags=R64.Flags(no_half_gradient=False))
    assert r.uv.tolist() == [[62.0, 30.0]]


def test_bilinear_and_validity_edges():
    img = np.arange(12, dtype=np.uint8).reshape(3, 4) * 10
    I = R64._Image(img)
    v, ok, _ = I.get(np.float32([0.5, 2.0, 2.0, -1e-7, 0.0]), np.float32([0.25, 3.0, 3.0000002, 0.0, np.nan]), R64.DEFAULT)
    assert v[0] == (0.5 * 0.75 * 0 + 0.5 * 0.25 * 10) + 0.5 * 0.75 * 40 + 0.5 * 0.25 * 50
    assert v[1] == 110.0 and ok.tolist() == [True, True, False, False, False]


def test_truncating_pyramid():
    img = np.array([[1, 2, 9], [3, 5, 9], [7, 7, 9]], np.uint8)
    lv = R64.create_pyramid(img, 2)
    assert lv[1].shape == (1, 1) and lv[1][0, 0] == (1 + 2 + 3 + 5) >> 2


def test_extended_patch_lattice():
    """ExtractExtendPatchInReferenceImage at (10.25, 20.5), half 1: a 5 x 5 lattice from floor - 2, with the position's own fractions."""
    img = (np.arange(40 * 40) % 251).reshape(40, 40).astype(np.uint8)
    o = R64.Options(kPatchRowHalfSize=1, kPatchColHalfSize=1)
    ex, exv, n = R64._ex_patch(R64._Image(img), np.float32([[10.25, 20.5]]), o, R64.DEFAULT)
    f = img.astype(np.float64)
    r, c = 18, 8
    want = ((0.5 * 0.75 * f[r, c] + 0.5 * 0.25 * f[r, c + 1]) + 0.5 * 0.75 * f[r + 1, c]) + 0.5 * 0.25 * f[r + 1, c + 1]
    assert n[0] == 25 and exv.all() and ex[0, 0] == want


def test_status_carry_cap_and_lssd_single_level_never_writes_back():
    rl, cl = scenes.scene(160, 120, 1, "easy", "translation")
    uv = scenes.features(40, 160, 120, half=4)
    st = np.zeros(40, np.uint8)
    st[3], st[4] = 3, 4
    for model in MODELS:
        r = R64.track_single(model, "inverse", rl[0], cl[0], uv, None, st, half=4, max_points=30)
        assert r.status[3] == 3 and r.status[4] == 4 and (r.uv[[3, 4]] == uv[[3, 4]]).all()
        assert (r.uv[30:] == uv[30:]).all() and (r.status[30:] == 0).all() and (r.iters[30:] == 0).all()
        if model == "lssd":
            assert (r.uv == uv).all() and (r.status[:30][st[:30] <= 1] == R64.TRACKED).sum() > 10
        else:
            assert (np.abs(r.uv[:30] - uv[:30] - [3.3, -2.1]).max(axis=1) < 0.2).sum() > 20


def test_affine_pyramid_path_ignores_the_prior():
    rl, cl = scenes.scene(160, 120, 2, "easy", "translation")
    uv = scenes.features(20, 160, 120, half=4)
    a = R64.track_pyramid("affine", "inverse", rl, cl, uv, half=4)
    b = R64.track_pyramid("affine", "inverse", rl, cl, uv, half=4, prior=np.float32([[1.2, 0.1], [0.0, 0.9]]))
    assert np.array_equal(a.uv, b.uv)


def test_flat_patch_is_singular_and_reported():
    rl, cl = scenes.scene(160, 120, 1, kind="flat")
    r = R64.track_single("basic", "inverse", rl[0], cl[0], np.float32([[80, 60]]), half=4)
    assert r.singular[0] and r.status[0] == R64.TRACKED and (r.uv[0] == [80, 60]).all()


# ---- 4. the tests can fail: mutants of ref64 ------------------------------------------------------------------------------------

MUTANTS = {
    # quirks switched off
    "half_gradient": (R64.Flags(no_half_gradient=False), VARIANTS, "one"),
    "affine_h34_y": (R64.Flags(affine_h34_yy=False), [("affine", k, False) for k in METHODS], "one"),
    "affine_pyramid_prior": (R64.Flags(affine_pyramid_identity=False), [("affine", k, False) for k in METHODS], "full"),
    "fast_no_status_reset": (R64.Flags(fast_status_reset=False), [(m, "fast", False) for m in MODELS] + [("lssd", "fast", True)], "full"),
    "lssd_no_mean": (R64.Flags(lssd_mean_normalise=False), [("lssd", "inverse", False), ("lssd", "direct", False)], "full"),
    "lssd_fast_matched_means": (R64.Flags(lssd_fast_luminance_mismatch=False), [("lssd", "fast", True)], "full"),
    "lssd_single_writes_back": (R64.Flags(lssd_single_no_writeback=False), [("lssd", k, False) for k in METHODS], "one"),
    # misreadings
    "gradient_other_image": (R64.Flags(gradient_other_image=True), [(m, k, False) for m in MODELS for k in ("inverse", "direct")], "one"),
    "cur_lattice_row_shift": (R64.Flags(cur_lattice_row_shift=1), VARIANTS, "one"),
    "swap_sr_sc": (R64.Flags(swap_sr_sc=True), VARIANTS, "one"),
    "validity_strict": (R64.Flags(validity_strict=True), [(m, k, False) for m in MODELS for k in ("inverse", "direct")] + [("affine", "fast", False)], "one"),
    "ex_patch_offset": (R64.Flags(ex_patch_offset=1), [(m, "fast", False) for m in MODELS], "one"),
}


MUTANT_CASES = {"one": ("example/6x6", "example/1x1", "similarity-hard/6x6", "odd-333x251/3x9", "small-64x48/6x6", "small-64x48/3x9",
                        "small-64x48/edge prediction"),
                "full": ("similarity-hard", "translation-hard", "similarity-hard/rect, options, prediction, status",
                         "similarity-hard/2 iterations", "small-160x120/2 iterations")}


def mutant_factor(oracle, flags, model, method, lum, kind):
    """The largest failure factor of the criterion over a few cases of `kind` (stops once it is past 1e3)."""
    worst = 0.0
    kinds = ["one-pyr"] if (kind == "one" and model == "lssd" and flags.lssd_single_no_writeback) else [kind]
    names = MUTANT_CASES[kind]
    for k in kinds:
        for case in _cases(k):
            if case[0] not in names:
                continue
            prior = PRIOR if flags.affine_pyramid_identity is False else None
            ref = run_ref(k, model, method, lum, case, flags=flags, prior=prior)
            c, s, it = run_oracle(oracle, k, model, method, lum, case, prior=prior)
            if kind == "one":
                ok, _, f, _ = one_step_check(model, ref, c, s, "")
            else:
                ok, _, f, stats = full_check(model, ref, c, s, it, "")
                f = max(f, stats["band_fraction"] / MAX_BAND)
            worst = max(worst, f if not ok or f > 1 else 0.0)
            if worst >= 1e3:
                return worst
    return worst


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_of_ref64_is_detected(oracle, name):
    flags, variants, kind = MUTANTS[name]
    factors = {}
    for model, method, lum in variants:
        factors[f"{model}/{method}{'+lum' if lum else ''}"] = mutant_factor(oracle, flags, model, method, lum, kind)
    print(f"\nMUTANT {name} ({kind}): " + ", ".join(f"{k} {v:.3g}" for k, v in factors.items()))
    assert all(f >= 10.0 for f in factors.values()), factors
