"""Sparse tracking from RAFT's coarse flow without a device: the scalar restatement (tests/flow_points_ref.c) pinned
against the existing contract (tests/flow_upsample_ref.c's fine field sampled with the three fmaf, bit for bit), against a float64
composition (float64 softmax, upsampling and bilinear), two mutants the float64 comparison must reject, one hand-built case per branch of
the status rules, and the loud failures of the Python entries.

Measured on the cases below (printed by the tests, -s shows them), in units of 2^-24 * max|8 flow|: the restatement's tracked points
against float64 at most MEASURED_UNITS; the bound is twice that."""
import functools
import types

import numpy as np
import pytest

from tests import flow_points_ref as P
from tests import flow_upsample_ref as R
from tests.test_flow_upsample_cpu import inputs, torch_upsample

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

GRIDS = [(1, 1, 1), (2, 3, 5), (1, 2, 33)]  # (B, H, W)
MASK_SCALES = (1.0, 0.25, 0.3)
LOGIT_SCALES = (1.0, 30.0)
SEEDS = (1, 2, 3, 4)
# max |cur_points - float64| over GRIDS x LOGIT_SCALES x SEEDS, full and cropped image, in units of 2^-24 * max|8 flow|; the
# asserted bound is twice it, for other seeds.  What the figure holds: the fine values' 3.31 units (tests/test_flow_upsample_cpu.py), three
# more roundings in the bilinear, and the rounding of ref + S, half an ulp of a coordinate of up to 8 W = 264 pixels.
MEASURED_UNITS = 4.70
UNITS = 2 * MEASURED_UNITS
NAN, INF = float("nan"), float("inf")


def fields(seed, B, H, W, logit_scale, flow_scale=0.4):
    """(flow, mask, flow_back, mask_back): the backward flow is minus the forward one plus a disturbance, so that forward-backward errors
    fall on both sides of a threshold of about a pixel."""
    flow, mask = (t.numpy() for t in inputs(seed, B, H, W, logit_scale, flow_scale))
    noise, mask_back = (t.numpy() for t in inputs(seed + 500, B, H, W, logit_scale, 0.1))
    return flow, mask, (-flow + noise).astype(np.float32), mask_back


def point_set(B, H, W, N, image_size, seed):
    """[B, N, 2] float32: first the points the kernel can get wrong, then seeded random ones, a fifth of them around the image's border
    on either side.  N below the count of special points keeps the first N of a seeded shuffle of them."""
    rows, cols = image_size
    rng = np.random.default_rng(seed)
    last_x, last_y = np.float32(cols - 1), np.float32(rows - 1)
    special = [(0, 0), (last_x, 0), (0, last_y), (last_x, last_y),                         # the four image corners
               (min(3, last_x), min(2, last_y)), (min(8, last_x), min(16, last_y)),         # whole-number coordinates
               (last_x, last_y * 0.37), (last_x * 0.61, last_y), (last_x - 0.25, last_y - 0.75) if min(rows, cols) > 1 else (0, 0),  # last column / row
               (-0.0, -0.0), (np.nextafter(last_x, np.float32(INF)), 0), (0, np.nextafter(last_y, np.float32(INF))),
               (-0.5, 1), (1, -1e-30), (cols, 0), (0, rows + 7), (-1e9, 3e9), (INF, 0), (0, -INF),  # outside
               (NAN, 0), (0, NAN), (NAN, NAN)]
    for k in sorted({0, 1, W // 2, W - 2, W - 1}):  # a corner pair in two coarse cells, at the zero-padded border too
        if 0 <= k and 8 * k + 7.5 <= cols - 1:
            special += [(8 * k + 7.5, last_y * 0.5), (8 * k + 7.5, 0), (8 * k + 7, last_y)]
    for k in sorted({0, 1, H - 2, H - 1}):
        if 0 <= k and 8 * k + 7.5 <= rows - 1:
            special += [(last_x * 0.5, 8 * k + 7.5), (0, 8 * k + 7.5), (last_x, 8 * k + 7.25)]
    special = np.float32(special)
    out = np.empty((B, N, 2), np.float32)
    for b in range(B):
        mine = special[rng.permutation(len(special))] if N < len(special) else special
        n_random = max(N - len(mine), 0)
        inner = rng.uniform(0, 1, (n_random, 2)) * [cols - 1, rows - 1]
        edge = rng.uniform(-1.5, 1.5, (n_random, 2)) + np.where(rng.uniform(size=(n_random, 2)) < 0.5, 0.0, [cols - 1, rows - 1])
        random = np.where(rng.uniform(size=(n_random, 1)) < 0.2, edge, inner).astype(np.float32)
        out[b] = np.concatenate([mine, random])[:N]
    return out


def image_sizes(H, W):
    """The whole grid, and an image the encoders would have rounded up to it."""
    return [(8 * H, 8 * W), (max(8 * H - 4, 1), max(8 * W - 3, 1))]


# ---- bit-identity with the existing contract -----------------------------------------------------------------------------------


def sample_dense_in_numpy(dense, points, image_size):
    """Steps 1 to 3 of DESIGN.md 5.17 on a stored fine field, in numpy float32 one operation at a time; the three fmaf are the
    restatement's own exported helper (numpy has no fused multiply-add).  Returns (cur_points, status)."""
    rows, cols = image_size
    B, _, H8, W8 = dense.shape
    last = np.float32([cols - 1, rows - 1])

    def inside(p):
        with np.errstate(invalid="ignore"):
            return (p[..., 0] >= 0) & (p[..., 0] <= last[0]) & (p[..., 1] >= 0) & (p[..., 1] <= last[1])

    live = inside(points)
    q = np.where(live[..., None], points, np.float32(0))
    p0 = np.floor(q)
    f = q - p0
    assert f.dtype == np.float32
    i0 = p0.astype(np.int64)
    ix1, iy1 = np.minimum(i0[..., 0] + 1, W8 - 1), np.minimum(i0[..., 1] + 1, H8 - 1)
    b = np.arange(B)[:, None]
    s = np.empty_like(q)
    for c in range(2):
        plane = dense[:, c]
        s[..., c] = P.bilinear(plane[b, i0[..., 1], i0[..., 0]], plane[b, i0[..., 1], ix1], plane[b, iy1, i0[..., 0]], plane[b, iy1, ix1], f[..., 0], f[..., 1])
    status = np.full(points.shape[:2], P.OUTSIDE, np.uint8)
    with np.errstate(all="ignore"):
        moved = points + s
    finite = np.isfinite(moved).all(-1)
    status[live & ~finite] = P.NUMERIC_ERROR
    cur = np.where((live & finite)[..., None], moved, points)
    status[live & finite & inside(cur)] = P.TRACKED
    return cur, status


@pytest.mark.parametrize("logit_scale", LOGIT_SCALES)
@pytest.mark.parametrize("B,H,W", GRIDS)
def test_bit_identical_to_the_upsampled_field_sampled(B, H, W, logit_scale):
    """The on-demand fine values are the floats flow_upsample_ref.upsample stores: tracking through (flow, mask) equals the restatement's
    rules on the stored field, and both equal the same rules written in numpy around the exported three-fmaf helper."""
    flow, mask, flow_back, mask_back = fields(10 * H + W, B, H, W, logit_scale)
    seen = set()
    for mask_scale in MASK_SCALES:
        dense, dense_back = R.upsample(flow, mask, mask_scale), R.upsample(flow_back, mask_back, mask_scale)
        for image_size in image_sizes(H, W):
            points = point_set(B, H, W, 150, image_size, 3)
            got = P.track(flow, mask, points, image_size, mask_scale)
            assert got[2] is None
            for want in (P.track_dense(dense, points, image_size), sample_dense_in_numpy(dense, points, image_size)):
                assert P.same(got[0], want[0]) and P.same(got[1], want[1])
            got = P.track(flow, mask, points, image_size, mask_scale, (flow_back, mask_back), 1.0)
            want = P.track_dense(dense, points, image_size, dense_back, 1.0)
            assert all(P.same(g, w) for g, w in zip(got, want))
            seen |= set(np.unique(got[1]).tolist())
    assert {P.TRACKED, P.OUTSIDE} <= seen and (min(H, W) == 1 or P.LARGE_RESIDUAL in seen)


def test_the_point_set_holds_what_it_promises():
    B, H, W = 2, 3, 5
    points = point_set(B, H, W, 150, (24, 40), 3)[0]
    with np.errstate(invalid="ignore"):
        assert np.isnan(points).any() and (points == points.round()).all(-1).any() and ((points[:, 0] % 8) == 7.5).any()
    for corner in ((0, 0), (39, 0), (0, 23), (39, 23)):
        assert (points == np.float32(corner)).all(-1).any()
    assert (points[:, 0] == 39).sum() >= 3 and (points[:, 1] == 23).sum() >= 3 and (points[:, 0] > 39).any() and (points[:, 0] < 0).any()
    assert point_set(B, H, W, 1, (24, 40), 3).shape == (B, 1, 2)


# ---- against float64 -----------------------------------------------------------------------------------------------------------


def float64_track(flow, mask, points, image_size):
    """float64 softmax and upsampling (model.py:48-64 by torch in float64), float64 bilinear with the clamped neighbour, ref + S in float64;
    rows of points that are not inside come back as NaN."""
    rows, cols = image_size
    with np.errstate(all="ignore"):
        dense = torch_upsample(torch.from_numpy(flow).double(), torch.from_numpy(mask).double()).numpy()
    B, _, H8, W8 = dense.shape
    p = points.astype(np.float64)
    live = (p[..., 0] >= 0) & (p[..., 0] <= cols - 1) & (p[..., 1] >= 0) & (p[..., 1] <= rows - 1)
    q = np.where(live[..., None], p, 0.0)
    p0 = np.floor(q)
    f = q - p0
    i0 = p0.astype(np.int64)
    ix1, iy1 = np.minimum(i0[..., 0] + 1, W8 - 1), np.minimum(i0[..., 1] + 1, H8 - 1)
    b = np.arange(B)[:, None]
    out = np.full(p.shape, np.nan)
    with np.errstate(all="ignore"):
        for c in range(2):
            plane = dense[:, c]
            top = plane[b, i0[..., 1], i0[..., 0]] * (1 - f[..., 0]) + plane[b, i0[..., 1], ix1] * f[..., 0]
            bot = plane[b, iy1, i0[..., 0]] * (1 - f[..., 0]) + plane[b, iy1, ix1] * f[..., 0]
            out[..., c] = np.where(live, p[..., c] + top * (1 - f[..., 1]) + bot * f[..., 1], np.nan)
    return out


def inside_points(B, N, image_size, seed):
    rng = np.random.default_rng(seed)
    rows, cols = image_size
    pts = (rng.uniform(0, 1, (B, N, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    pts[:, :4] = np.float32([(cols - 1, 0), (cols - 1, rows - 1), (0, rows - 1), (cols - 1, (rows - 1) * 0.5)])  # the clamp
    return pts


@functools.lru_cache(maxsize=None)
def float64_case(k, logit_scale, seed, cropped):
    """(flow, mask, points, image_size, float64 tracked points, unit) — computed once, shared, never written to."""
    B, H, W = GRIDS[k]
    flow, mask = (t.numpy() for t in inputs(200 + 10 * k + seed, B, H, W, logit_scale))
    image_size = image_sizes(H, W)[int(cropped)]
    points = inside_points(B, 200, image_size, seed)
    return flow, mask, points, image_size, float64_track(flow, mask, points, image_size), 2.0 ** -24 * float(np.abs(8 * flow).max())


def units_off(cur, ref64, unit):
    """The largest error of the tracked points in units; a non-finite point where float64 has a finite one is infinitely far."""
    with np.errstate(invalid="ignore"):
        d = np.abs(cur.astype(np.float64) - ref64)
    d[~np.isfinite(cur) & np.isfinite(ref64)] = np.inf
    return float(np.nanmax(d)) / unit


def all_float64_cases(seeds=SEEDS):
    return [(k, s, seed, c) for k in range(len(GRIDS)) for s in LOGIT_SCALES for seed in seeds for c in (False, True)]


def test_restatement_against_float64():
    worst = {}
    for key in all_float64_cases(SEEDS + (5,)):
        flow, mask, points, image_size, ref64, unit = float64_case(*key)
        worst[key] = units_off(P.track(flow, mask, points, image_size)[0], ref64, unit)
    measured = max(v for key, v in worst.items() if key[2] in SEEDS)
    print(f"restatement vs float64: {measured:.2f} units over the measured seeds, {max(worst.values()):.2f} with a fifth seed (recorded "
          f"{MEASURED_UNITS}, bound {UNITS})")
    assert measured <= MEASURED_UNITS * 1.0001, "the recorded maximum is out of date"
    assert measured >= MEASURED_UNITS * 0.99, "the recorded maximum is out of date"
    assert max(worst.values()) <= UNITS


def hostile_last_column():
    """Grid (1, 2, 33) with an infinite flow in coarse column 0 and points in the grid's last column and last row.  float64 and the
    contract never read column 0 from there.  A neighbour that wraps does, and although its weight fx is exactly 0 in the last column
    (u = 8 W - 1 is a whole number: for finite fields the wrapped and the clamped neighbour give the same bits), 0 * inf is NaN: the clamp
    is what keeps the last column and row independent of the far side of the grid."""
    B, H, W = GRIDS[2]
    flow, mask = (t.numpy().copy() for t in inputs(77, B, H, W, 1.0))
    flow[:, :, :, 0] = INF
    image_size = (8 * H, 8 * W)
    points = inside_points(B, 40, image_size, 9)
    points[:, :, 0] = 8 * W - 1
    return flow, mask, points, image_size, float64_track(flow, mask, points, image_size), 2.0 ** -24 * float(np.abs(8 * flow[:, :, :, 1:]).max())


@pytest.mark.parametrize("variant", [P.MUTANT_SWAPPED_UV, P.MUTANT_WRAPPED_NEIGHBOUR], ids=["(u, v) read as (v, u)", "neighbour wrapped"])
def test_mutants_fail_the_float64_comparison(variant):
    """The comparison has teeth: each mutant misses the bound on inputs where the contract meets it."""
    if variant == P.MUTANT_SWAPPED_UV:
        cases = [float64_case(*key) for key in all_float64_cases((1,))]
    else:
        cases = [hostile_last_column()]
    contract = [units_off(P.track(f, m, p, size)[0], ref64, unit) for f, m, p, size, ref64, unit in cases]
    mutant = [units_off(P.track(f, m, p, size, variant=variant)[0], ref64, unit) for f, m, p, size, ref64, unit in cases]
    print(f"mutant {variant}: {['%.3g' % w for w in mutant]} units, the contract {['%.3g' % w for w in contract]} (bound {UNITS})")
    assert max(contract) <= UNITS
    assert min(mutant) > UNITS
    if variant == P.MUTANT_WRAPPED_NEIGHBOUR:  # and on finite fields it is the contract, bit for bit
        f, m, p, size, _, _ = float64_case(2, 1.0, 1, False)
        assert all(P.same(a, b) for a, b in zip(P.track(f, m, p, size, variant=variant)[:2], P.track(f, m, p, size)[:2]))


# ---- the status table ----------------------------------------------------------------------------------------------------------

SIDE = 8  # an 8 x 8 coarse grid: 64 x 64 fine pixels


def uniform_field(dx, dy):
    """A flow of exactly (dx, dy) fine pixels everywhere: the centre logit at +200 gives weight 1 on the coarse pixel itself and 0 on
    its neighbours, so every fine value is 8 * flow = (dx, dy) and every bilinear sample is too."""
    flow = np.empty((1, 2, SIDE, SIDE), np.float32)
    flow[0, 0], flow[0, 1] = dx / 8, dy / 8
    mask = np.zeros((1, 576, SIDE, SIDE), np.float32)
    mask[0, 4 * 64:5 * 64] = 200.0
    return flow, mask


def one(flow, mask, point, image=64, backward=None, t=0.0):
    cur, status, e2 = P.track(flow, mask, np.float32([[point]]), (image, image), 1.0, backward, t)
    return cur[0, 0], int(status[0, 0]), (None if e2 is None else e2[0, 0])


def bits(a):
    return np.float32(a).view(np.uint32).tolist()


def test_status_table_reference_points():
    flow, mask = uniform_field(2.0, -1.0)
    back = uniform_field(-2.0, 1.0)
    for ref in ((NAN, 5.0), (5.0, NAN), (np.float32(np.nextafter(np.float32(63), np.float32(INF))), 5.0), (5.0, 64.0), (-1e-45, 5.0)):
        cur, status, e2 = one(flow, mask, ref, backward=back)
        assert status == P.OUTSIDE and bits(cur) == bits(ref) and bits(e2) == bits(0.0), ref
    cur, status, _ = one(flow, mask, (-0.0, 5.0))  # -0 is inside
    assert status == P.TRACKED and cur.tolist() == [2.0, 4.0]
    still = uniform_field(0.0, 0.0)
    cur, status, _ = one(*still, (63.0, 63.0))  # image_cols - 1 exactly is inside
    assert status == P.TRACKED and cur.tolist() == [63.0, 63.0]


def test_status_table_forward_step():
    flow, mask = uniform_field(10.0, 0.0)
    cur, status, e2 = one(flow, mask, (60.0, 5.0), backward=uniform_field(-10.0, 0.0))  # carried out of the image: as computed, no check
    assert status == P.OUTSIDE and cur.tolist() == [70.0, 5.0] and bits(e2) == bits(0.0)
    for value in (INF, -INF, NAN):
        flow, mask = uniform_field(1.0, 1.0)
        flow[0, 0, 2, 3] = value
        cur, status, _ = one(flow, mask, (8 * 3 + 2.5, 8 * 2 + 1.5))
        assert status == P.NUMERIC_ERROR and cur.tolist() == [26.5, 17.5], value
        assert one(flow, mask, (50.0, 50.0))[1] == P.TRACKED  # far from it
    flow, mask = uniform_field(1.0, 1.0)  # an image smaller than its grid: pixel 61 exists in the grid and is outside a 60 x 60 image
    assert one(flow, mask, (61.0, 5.0), image=60)[1] == P.OUTSIDE and one(flow, mask, (61.0, 5.0), image=64)[1] == P.TRACKED
    cur, status, _ = one(flow, mask, (58.5, 5.0), image=60)  # 59.5 > 59: carried out of the image, inside the grid
    assert status == P.OUTSIDE and cur.tolist() == [59.5, 6.0]


def test_status_table_forward_backward():
    flow, mask = uniform_field(2.0, -1.0)
    cur, status, e2 = one(flow, mask, (10.25, 20.0), backward=uniform_field(-2.0, 1.0), t=0.0)  # returns exactly: 0 <= 0 * 0
    assert status == P.TRACKED and cur.tolist() == [12.25, 19.0] and bits(e2) == bits(0.0)
    near = uniform_field(-1.5, 1.0)  # comes back 0.5 pixels off: e2 = 0.25 exactly
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    cur, status, e2 = one(flow, mask, (10.25, 20.0), backward=near, t=below)
    assert status == P.LARGE_RESIDUAL and cur.tolist() == [12.25, 19.0] and e2 == 0.25  # e2 just above t * t
    assert one(flow, mask, (10.25, 20.0), backward=near, t=0.5)[1] == P.TRACKED
    bad = uniform_field(-2.0, 1.0)
    bad[0][0, 1, 2, 1] = NAN  # the coarse pixel of (12.25, 19)
    cur, status, e2 = one(flow, mask, (10.25, 20.0), backward=bad, t=1e30)
    assert status == P.LARGE_RESIDUAL and cur.tolist() == [12.25, 19.0] and np.isnan(e2)
    assert P.track(flow, mask, np.float32([[(10.25, 20.0)]]), (64, 64))[2] is None


# ---- loud failures, before any device is touched -------------------------------------------------------------------------------


def test_wrapper_refuses_bad_arguments_without_a_device():
    import feature_tracker_amd as F
    flow, mask, pts = torch.zeros(2, 2, 3, 5), torch.zeros(2, 576, 3, 5), torch.zeros(2, 7, 2)
    size = (24, 40)
    bad = [
        ("flow must be", (flow.double(), mask, pts, size)), ("mask must be", (flow, mask.half(), pts, size)), ("flow must be", (flow[0], mask, pts, size)),
        ("mask must be", (flow, torch.zeros(2, 575, 3, 5), pts, size)), ("agree", (flow, torch.zeros(2, 576, 4, 5), pts, size)),
        ("flow must be", (flow.numpy(), mask, pts, size)),
        ("points must be", (flow, mask, pts.double(), size)), ("points must be", (flow, mask, pts[0], size)), ("points must be", (flow, mask, torch.zeros(2, 7, 3), size)),
        ("points must be", (flow, mask, torch.zeros(3, 7, 2), size)), ("points must be", (flow, mask, pts.numpy(), size)),
        ("image_size", (flow, mask, pts, (25, 40))), ("image_size", (flow, mask, pts, (24, 41))), ("image_size", (flow, mask, pts, (0, 40))),
        ("image_size", (flow, mask, pts, 24)), ("image_size", (flow, mask, pts, (24, 40, 1))),
        ("mask_scale", (flow, mask, pts, size, NAN)), ("mask_scale", (flow, mask, pts, size, INF)),
        ("go together", (flow, mask, pts, size, 1.0, (flow, mask))), ("go together", (flow, mask, pts, size, 1.0, None, 1.0)),
        ("backward must be", (flow, mask, pts, size, 1.0, flow, 1.0)), ("backward\\[1\\] must be", (flow, mask, pts, size, 1.0, (flow, flow), 1.0)),
        ("agree", (flow, mask, pts, size, 1.0, (torch.zeros(2, 2, 3, 6), mask), 1.0)),
        ("forward_backward", (flow, mask, pts, size, 1.0, (flow, mask), -1.0)), ("forward_backward", (flow, mask, pts, size, 1.0, (flow, mask), NAN)),
        ("forward_backward", (flow, mask, pts, size, 1.0, (flow, mask), INF)),
    ]
    for match, args in bad:
        with pytest.raises(ValueError, match=match):
            F.track_points_from_flow(*args)
    with pytest.raises(RuntimeError, match="inference only"):
        F.track_points_from_flow(flow, mask, pts.clone().requires_grad_(True), size)
    with pytest.raises(ValueError, match="no CPU fallback"):
        F.track_points_from_flow(flow, mask, pts, size)
    with pytest.raises(ValueError, match="no CPU fallback"):
        F.track_points_from_flow(flow, mask, pts, size, 0.25, (flow, mask), 1.5)


def test_raft_track_points_refuses_bad_arguments_without_a_device(monkeypatch):
    """The checks of Raft.__call__ and those of the points, every one before the first launch: the recording library sees none."""
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from tests.test_raft_encoder_cpu import RAFT_CASES, make_image, make_raft_state
    c = RAFT_CASES[0]
    model = F.Raft.from_state_dict(make_raft_state(c, 1), c[3], c[4], max_iterations=2)
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    ref, cur, pts = make_image(1, 1, 16, 24, 1), make_image(1, 1, 16, 24, 2), torch.zeros(1, 5, 2)
    for match, args, kwargs in (
            ("ref_image must be", (ref.double(), cur, pts), {}), ("cur_image must be", (ref, cur[0], pts), {}),
            ("The size of the reference and current images should be the same", (ref, cur[:, :, :15], pts), {}),
            ("iterations 0", (ref, cur, pts), {"iterations": 0}),
            ("points must be", (ref, cur, pts.double()), {}), ("points must be", (ref, cur, pts[0]), {}), ("points must be", (ref, cur, torch.zeros(2, 5, 2)), {}),
            ("points must be", (ref, cur, torch.zeros(1, 5, 3)), {}), ("points must be", (ref, cur, pts.numpy()), {}),
            ("forward_backward", (ref, cur, pts), {"forward_backward": -0.5}), ("forward_backward", (ref, cur, pts), {"forward_backward": NAN}),
            ("forward_backward", (ref, cur, pts), {"forward_backward": INF}),
            ("no CPU fallback", (ref, cur, pts), {}), ("no CPU fallback", (ref, cur, pts), {"forward_backward": 1.0, "return_error": True})):
        with pytest.raises(ValueError, match=match):
            model.track_points(*args, **kwargs)
    with pytest.raises(RuntimeError, match="Raft is inference only"):
        model.track_points(ref, cur, pts.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="no CPU fallback"):
        model.update_block(torch.zeros(1, c[0], 2, 3), torch.zeros(1, c[2], 2, 3), torch.zeros(1, 9, 2, 3), torch.zeros(1, 2, 2, 3), want_mask=False)
    assert recorder.calls == []


def test_device_entry_refuses_bad_arguments_without_a_device():
    from feature_tracker_amd import device as D
    ctx = types.SimpleNamespace(handle=None)
    flow, mask, pts = torch.zeros(1, 2, 3, 5), torch.zeros(1, 576, 3, 5), torch.zeros(1, 4, 2)
    cur, status = torch.zeros(1, 4, 2), torch.zeros(1, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="^flow must be a CUDA tensor"):
        D.flow_track_points_device(ctx, flow, mask, pts, 24, 40, cur, status)
    with pytest.raises(ValueError, match="^flow must be .*wrong dtype"):
        D.flow_track_points_device(ctx, flow.double(), mask, pts, 24, 40, cur, status)
    with pytest.raises(ValueError, match="mask_scale"):
        D.flow_track_points_device(ctx, flow, mask, pts, 24, 40, cur, status, mask_scale=NAN)
    for t in (-1.0, NAN):
        with pytest.raises(ValueError, match="fb_threshold"):
            D.flow_track_points_device(ctx, flow, mask, pts, 24, 40, cur, status, fb_threshold=t)
    with pytest.raises(ValueError, match="go together"):
        D.flow_track_points_device(ctx, flow, mask, pts, 24, 40, cur, status, flow_back=flow)


# the walk of tests/args_walk.py (duck-typed tensors, a recording stand-in for the native library) over this entry
def _walk_call(w, rows=24, cols=40):
    from feature_tracker_amd import device as D
    return D.flow_track_points_device(w.ctx, w.t("flow", "float32", 2, 2, 3, 5), w.t("mask", "float32", 2, 576, 3, 5), w.t("points", "float32", 2, 9, 2), rows,
                                      cols, w.t("cur_points", "float32", 2, 9, 2), w.t("status", "uint8", 2, 9), w.t("fb_error2", "float32", 2, 9), 0.25,
                                      w.t("flow_back", "float32", 2, 2, 3, 5), w.t("mask_back", "float32", 2, 576, 3, 5), 1.5)


def test_device_entry_takes_no_pointer_of_an_unchecked_argument(monkeypatch):
    A.walk_call(monkeypatch, _walk_call, ["ftk_flow_track_points_device"])


@pytest.mark.parametrize("which,change,match", [
    (0, ("dtype", "float64"), "flow must be"), (1, ("dtype", "float64"), "mask must be"), (2, ("dtype", "float64"), "points must be"),
    (3, ("dtype", "float64"), "cur_points must be"), (4, ("dtype", "float32"), "status must be"), (5, ("dtype", "float64"), "fb_error2 must be"),
    (6, ("dtype", "float64"), "flow_back must be"), (7, ("dtype", "float64"), "mask_back must be"),
    (1, ("shape", (2, 575, 3, 5)), "mask must be.*dimension 1 is 575, not 576"), (2, ("shape", (2, 9, 3)), "points must be.*dimension 2 is 3, not 2"),
    (2, ("shape", (3, 9, 2)), "points must be.*dimension 0"), (3, ("shape", (2, 8, 2)), "cur_points must be.*dimension 1 is 8, not 9"),
    (4, ("shape", (2, 9, 1)), "status must be.*3 dimensions instead of 2"), (5, ("shape", (2, 10)), "fb_error2 must be.*dimension 1"),
    (6, ("shape", (2, 2, 3, 6)), "flow_back must be.*dimension 3"), (7, ("shape", (2, 576, 4, 5)), "mask_back must be.*dimension 2"),
    (2, ("device", 1), "points must be on cuda:0"), (4, ("device", 1), "status must be on cuda:0"),
])
def test_device_entry_stops_before_the_library(monkeypatch, which, change, match):
    A.refused_call(monkeypatch, _walk_call, (which, *change), match)


@pytest.mark.parametrize("rows,cols", [(25, 40), (24, 41), (0, 40), (24, -1)])
def test_device_entry_refuses_an_image_outside_the_grid(monkeypatch, rows, cols):
    w = A.Walk(monkeypatch)
    with pytest.raises(ValueError, match="image_rows x image_cols"):
        _walk_call(w, rows, cols)
    assert w.lib.calls == [] and w.unchecked_reads == []


def test_header_library_and_binding_agree():
    import os
    import re

    from feature_tracker_amd import _native as N
    header = open(os.path.join(os.path.dirname(N.CSRC_DIR), "..", "include", "ftk.h")).read()
    assert int(re.search(r"#define FTK_FLOW_POINTS_TILE (\d+)", header).group(1)) == N.FTK_FLOW_POINTS_TILE
    assert "ftk_flow_track_points_device" in N.EXPORTS
    values = dict(re.findall(r"(FTK_(?:NOT_TRACKED|TRACKED|LARGE_RESIDUAL|OUTSIDE|NUMERIC_ERROR)) = (\d)", header))
    assert [int(values["FTK_" + n]) for n in ("NOT_TRACKED", "TRACKED", "LARGE_RESIDUAL", "OUTSIDE", "NUMERIC_ERROR")] == \
        [P.NOT_TRACKED, P.TRACKED, P.LARGE_RESIDUAL, P.OUTSIDE, P.NUMERIC_ERROR]
