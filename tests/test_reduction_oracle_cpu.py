"""CPU tests of the wide-sum oracle (oracle/liboracle_sum64.so, oracle_lib.wide()): the reference for the trackers' throughput
(tree) reduction mode in tests/test_reduction_tree_gpu.py.

- On integer-exact scenes every summation order gives the same float sums: the wide build must equal the default build bit for bit.
- Off them, its sums are the correctly rounded sums of the default build's own f32 products: checked against math.fsum of those
  products, restated in numpy, for Basic KLT inverse.
- Negative control: a wide build that loses every 64-th pixel's terms (what a reduction that drops one lane's partial does) fails
  the GPU tests' acceptance criterion by a wide margin on the same scenes."""
import math

import numpy as np
import pytest

from tests import oracle_lib, scenes

MODELS = ["basic", "affine", "lssd"]
METHODS = ["inverse", "direct", "fast"]


@pytest.fixture(scope="module")
def wide():
    w = oracle_lib.wide()
    w.drop_stride(0)
    yield w
    w.drop_stride(0)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("model", ["basic", "affine"])  # (LSSD divides by its patch means: not integer-exact)
@pytest.mark.parametrize("method", METHODS)
def test_wide_build_equals_default_build_on_integer_exact_scenes(wide, model, method):
    w, h = (320, 240) if model != "affine" else (32, 24)
    lo, hi = (100, 160) if model != "affine" else (126, 130)
    flat = (w * 5 // 8, h * 5 // 8, w * 15 // 16, h * 15 // 16)
    ref, cur = scenes.integer_scene(w, h, lo, hi, flat=flat)
    assert scenes.integer_sum_bound(model, ref, cur, 6, 6) < 2 ** 24
    uv = scenes.integer_features(120, w, h, 6, flat=flat)
    # one step: the next one starts from a non-integer position, where the scene is no longer integer-exact
    a = oracle_lib.klt_track_pyramid(model, [ref], [cur], uv, method=method, half=6, max_iteration=1)
    b = wide.klt_track_pyramid(model, [ref], [cur], uv, method=method, half=6, max_iteration=1)
    assert a[0] == b[0] and _bits_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), (model, method)
    assert not _bits_equal(a[1], uv), "the scene must move the features"


def test_wide_build_equals_default_build_on_an_integer_exact_direct_problem(wide):
    """The direct method's 27 sums at one iteration: points on the plane z = 1 at integer (x, y) in [-5, 5] with fx = fy = 1 make every
    Jacobian entry an integer, the central differences are halves (values in [127, 129]): every product is a multiple of 1/4 and
    every partial sum stays far below 2^22."""
    ref, cur = scenes.integer_scene(24, 24, 127, 129, shift=(1, 0))
    xs, ys = np.meshgrid(np.arange(-5, 6, 2), np.arange(-5, 6, 2))
    pts = np.stack([xs.ravel(), ys.ravel(), np.ones(xs.size)], axis=1).astype(np.float32)
    K = [1.0, 1.0, 12.0, 12.0]
    uv = (pts[:, :2] + np.float32(12.0)).astype(np.float32)
    # bound: |jac_k| <= |gx J0k| + |gy J1k| <= 2 * 26 (|g| <= 1, |J| <= 1 + 5^2); 36 features x 25 pixels of quarter-integers
    assert 36 * 25 * 52 ** 2 < 2 ** 22
    a = oracle_lib.direct_track([ref], [cur], K, pts, uv, half=2, max_points=500, max_iteration=1)
    b = wide.direct_track([ref], [cur], K, pts, uv, half=2, max_points=500, max_iteration=1)
    assert _bits_equal(a[2], b[2]) and _bits_equal(a[3], b[3]) and _bits_equal(a[1], b[1])
    assert not _bits_equal(a[3], np.zeros(3)), "the problem must move the pose"


def _bilinear32(img, row, col):
    """orc_bilinear in float32, the same operations in the same order (oracle_internal.h)."""
    f = np.float32
    r0, c0 = int(row), int(col)
    sr = f(row) - f(math.floor(row))
    sc = f(col) - f(math.floor(col))
    r1 = min(r0 + 1, img.shape[0] - 1)
    c1 = min(c0 + 1, img.shape[1] - 1)
    isr, isc = f(1) - sr, f(1) - sc
    w_tl, w_tr, w_bl, w_br = isr * isc, isr * sc, sr * isc, sr * sc
    return ((w_tl * f(img[r0, c0]) + w_tr * f(img[r0, c1])) + w_bl * f(img[r1, c0])) + w_br * f(img[r1, c1])


def _basic_inverse_step_fsum(ref, cur, u, v, half):
    """One Basic-KLT inverse step (oracle_basic_klt.c): the f32 products, summed exactly (math.fsum), solved in float64."""
    f = np.float32
    rows, cols = ref.shape
    inside = lambda r, c: 0.0 <= r <= rows - 1 and 0.0 <= c <= cols - 1
    terms = [[], [], [], [], []]
    for drow in range(-half, half + 1):
        for dcol in range(-half, half + 1):
            ri, ci = f(drow) + f(v), f(dcol) + f(u)
            taps = [(ri, ci - f(1)), (ri, ci + f(1)), (ri - f(1), ci), (ri + f(1), ci), (ri, ci)]
            if not all(inside(r, c) for r, c in taps):
                continue
            left, right, top, bottom, i_ref = (_bilinear32(ref, r, c) for r, c in taps)
            i_cur = _bilinear32(cur, ri, ci)
            fx, fy, ft = right - left, bottom - top, i_cur - i_ref
            for k, t in enumerate((fx * fx, fy * fy, fx * fy, -(fx * ft), -(fy * ft))):
                terms[k].append(float(t))
    s = [math.fsum(t) for t in terms]
    step = np.linalg.solve(np.array([[s[0], s[2]], [s[2], s[1]]]), np.array([s[3], s[4]]))
    return np.float64(u) + step[0], np.float64(v) + step[1]


def test_wide_build_is_at_least_as_close_to_exact_sums_as_the_f32_chain(wide):
    """Non-integer positions near the origin (small ulp of the result), 31 x 31 patches (961-term chains) on the textured scene."""
    ref_levels, cur_levels = scenes.scene(320, 240, 1)
    ref, cur = ref_levels[0], cur_levels[0]
    rs = np.random.RandomState(4)
    uv = np.stack([rs.uniform(17.0, 30.0, 12), rs.uniform(17.0, 30.0, 12)], axis=1).astype(np.float32)
    _, c32, _, _ = oracle_lib.klt_track_pyramid("basic", [ref], [cur], uv, method="inverse", half=15, max_iteration=1)
    _, c64, _, _ = wide.klt_track_pyramid("basic", [ref], [cur], uv, method="inverse", half=15, max_iteration=1)
    exact = np.array([_basic_inverse_step_fsum(ref, cur, u, v, 15) for u, v in uv])
    e32 = np.abs(c32.astype(np.float64) - exact).max(axis=1)
    e64 = np.abs(c64.astype(np.float64) - exact).max(axis=1)
    assert e64.sum() <= e32.sum() and e64.max() <= e32.max(), (e64, e32)
    assert (e64 <= 2 * np.spacing(np.float32(32.0))).all(), e64
    assert not np.array_equal(c32, c64), "the scene must make the f32 chain's rounding visible"


def _regime_scenes():
    ref_levels, cur_levels = scenes.scene(320, 240, 1)
    yield "synthetic", ref_levels[0], cur_levels[0], scenes.features(600, 320, 240, half=6)
    import os
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ref = np.array(Image.open(os.path.join(root, "tests", "data", "optical_flow", "ref_image.png")).convert("L"), dtype=np.uint8)
    cur = np.array(Image.open(os.path.join(root, "tests", "data", "optical_flow", "cur_image.png")).convert("L"), dtype=np.uint8)
    rs = np.random.RandomState(5)
    uv = np.stack([rs.uniform(30, ref.shape[1] - 30, 600), rs.uniform(30, ref.shape[0] - 30, 600)], axis=1).astype(np.float32)
    yield "real pair", ref, cur, uv


@pytest.mark.parametrize("model,method", [("basic", "inverse"), ("basic", "fast"), ("lssd", "inverse"), ("affine", "fast")])
def test_negative_control_a_lost_lane_partial_fails_the_criterion(wide, model, method):
    """drop_stride(64) stands in for a tree reduction that loses a lane's partial: on the GPU test's scenes the criterion must reject
    it by a factor of at least 10 (and accept the wide build itself)."""
    for name, ref, cur, uv in _regime_scenes():
        _, c_exact, _, _ = oracle_lib.klt_track_pyramid(model, [ref], [cur], uv, method=method, half=6, max_iteration=1)
        _, c_wide, _, _ = wide.klt_track_pyramid(model, [ref], [cur], uv, method=method, half=6, max_iteration=1)
        try:
            wide.drop_stride(64)
            _, c_drop, _, _ = wide.klt_track_pyramid(model, [ref], [cur], uv, method=method, half=6, max_iteration=1)
        finally:
            wide.drop_stride(0)
        ok, msg, ratio = scenes.rounding_regime(c_wide, c_exact, c_wide, name)
        assert ok, msg
        ok, msg, ratio = scenes.rounding_regime(c_drop, c_exact, c_wide, f"{name} {model}/{method} drop 64")
        print(msg, f"ratio {ratio:.1f}")
        assert not ok and ratio > 10.0, msg


def test_negative_control_on_the_direct_method(wide):
    from tests.test_direct_method_gpu import CX, CY, FX, FY, scene
    rl, cl, uv, pts = scene(levels=1, n=300)
    K = [FX, FY, CX, CY]
    a = oracle_lib.direct_track(rl, cl, K, pts, uv, max_points=300, max_iteration=1)
    b = wide.direct_track(rl, cl, K, pts, uv, max_points=300, max_iteration=1)
    try:
        wide.drop_stride(64)
        d = wide.direct_track(rl, cl, K, pts, uv, max_points=300, max_iteration=1)
    finally:
        wide.drop_stride(0)
    pose = lambda r: np.concatenate([r[2], r[3]])[None, :]
    ok, msg, _ = scenes.rounding_regime(pose(b), pose(a), pose(b), "direct wide")
    assert ok, msg
    ok, msg, ratio = scenes.rounding_regime(pose(d), pose(a), pose(b), "direct drop 64")
    print(msg, f"ratio {ratio:.1f}")
    assert not ok and ratio > 10.0, msg
