"""track_points_from_flow on the device against the scalar restatement (tests/flow_points_ref.c): tracked points, status and
forward-backward error bit-identical on every grid, point count around the kernel's tile and image size, with and without the backward
pair, on ordinary and hostile logits (any NaN equals any NaN); the same bits as sampling upsample_flow's device output;
and the entry's handling of strided points, of a second device and of arguments the C entry refuses."""
import numpy as np
import pytest

from tests import flow_points_ref as P
from tests.test_flow_points_cpu import GRIDS, fields, image_sizes, point_set
from tests.test_flow_upsample_cpu import hostile_inputs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from feature_tracker_amd import _native as N  # noqa: E402

T = N.FTK_FLOW_POINTS_TILE
COUNTS = (1, T - 1, T, T + 1, 2 * T + 3)
MASK_SCALES = (1.0, 0.25, 0.3)


def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def device_track(ftk, flow, mask, points, image_size, mask_scale=1.0, backward=None, t=None):
    back = None if backward is None else tuple(on_device(a) for a in backward)
    cur, status, e2 = ftk.track_points_from_flow(on_device(flow), on_device(mask), on_device(points), image_size, mask_scale, back, t)
    assert cur.dtype == torch.float32 and status.dtype == torch.uint8 and (e2 is None) == (backward is None)
    return cur.cpu().numpy(), status.cpu().numpy(), None if e2 is None else e2.cpu().numpy()


def explain(got, want, points):
    for name, g, w in zip(("cur_points", "status", "fb_error2"), got, want):
        if w is not None and not P.same(g, w):
            where = np.argwhere((g != w) & ~(np.isnan(g) & np.isnan(w)) if g.dtype == np.float32 else g != w)[:4]
            return f"{name} differs at {where.tolist()}: points {[points[tuple(i[:2])].tolist() for i in where]}, got {[g[tuple(i)].item() for i in where]}, " \
                   f"want {[w[tuple(i)].item() for i in where]}"
    return None


@pytest.mark.parametrize("with_backward", [False, True], ids=["forward", "forward-backward"])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("B,H,W", GRIDS)
def test_bit_identical_to_the_restatement(ftk, B, H, W, count, with_backward):
    """Logit scale 30 puts x - m across exp_c's cutoff; mask_scale 0.3 is no power of two; the cropped image is one the encoders rounded up."""
    seen = set()
    for n, image_size in enumerate(image_sizes(H, W)):
        logit_scale, mask_scale = (1.0, 30.0)[n], MASK_SCALES[(n + count) % 3]
        flow, mask, flow_back, mask_back = fields(100 * H + W + count, B, H, W, logit_scale)
        points = point_set(B, H, W, count, image_size, count)
        backward, t = ((flow_back, mask_back), 1.0) if with_backward else (None, None)
        got = device_track(ftk, flow, mask, points, image_size, mask_scale, backward, t)
        want = P.track(flow, mask, points, image_size, mask_scale, backward, 1.0)
        assert got[0].shape == (B, count, 2) and got[1].shape == (B, count)
        assert explain(got, want, points) is None, explain(got, want, points)
        seen |= set(np.unique(want[1]).tolist())
    if count >= T - 1:
        assert {P.TRACKED, P.OUTSIDE} <= seen


@pytest.mark.parametrize("with_backward", [False, True], ids=["forward", "forward-backward"])
def test_hostile_logits(ftk, with_backward):
    """NaN at k = 0 and at k = 5, +inf, nine -inf, one -inf, x - m on both sides of the cutoff (tests/test_flow_upsample_cpu.py), in the
    forward pair and, with the check, in the backward pair too: NUMERIC_ERROR, NaN errors and ordinary points side by side."""
    flow, mask = hostile_inputs()
    flow = (flow * np.float32(0.1)).astype(np.float32)  # most points stay inside the 24 x 72 image
    B, _, H, W = flow.shape
    image_size = (8 * H, 8 * W)
    ys, xs = np.meshgrid(np.arange(6.5, 23, 1.75, dtype=np.float32), np.arange(0, 8 * W - 1, 2.25, dtype=np.float32), indexing="ij")
    points = np.concatenate([point_set(B, H, W, 100, image_size, 5), np.stack([xs.ravel(), ys.ravel()], -1)[None]], 1)
    # the backward pair's hostile logits lie one coarse row lower, where the forward pair is ordinary: points arrive there alive
    backward, t = (((-flow).astype(np.float32), np.roll(mask, 1, axis=2)), 0.75) if with_backward else (None, None)
    got = device_track(ftk, flow, mask, points, image_size, 1.0, backward, t)
    want = P.track(flow, mask, points, image_size, 1.0, backward, 0.75)
    assert {P.TRACKED, P.OUTSIDE, P.NUMERIC_ERROR} <= set(np.unique(want[1]).tolist())
    if with_backward:
        assert P.LARGE_RESIDUAL in want[1] and np.isnan(want[2]).any() and not np.isnan(want[2]).all()
    assert explain(got, want, points) is None, explain(got, want, points)


@pytest.mark.parametrize("B,H,W", GRIDS)
def test_same_bits_as_sampling_the_upsampled_flow(ftk, B, H, W):
    """upsample_flow's device output, copied to the host and sampled at the points by the restatement's rules, is what the kernel gives
    without ever storing it."""
    flow, mask, flow_back, mask_back = fields(7 * H + W, B, H, W, 1.0)
    for mask_scale, image_size in zip((0.3, 1.0), image_sizes(H, W)):
        points = point_set(B, H, W, 2 * T + 3, image_size, 11)
        dense, dense_back = (ftk.upsample_flow(on_device(f), on_device(m), mask_scale).cpu().numpy() for f, m in ((flow, mask), (flow_back, mask_back)))
        got = device_track(ftk, flow, mask, points, image_size, mask_scale, (flow_back, mask_back), 1.0)
        want = P.track_dense(dense, points, image_size, dense_back, 1.0)
        assert explain(got, want, points) is None, explain(got, want, points)
        got = device_track(ftk, flow, mask, points, image_size, mask_scale)
        want = P.track_dense(dense, points, image_size)
        assert explain(got, want, points) is None, explain(got, want, points)


def test_no_points_and_batch_stacking(ftk):
    B, H, W = 4, 3, 5
    flow, mask, _, _ = fields(3, B, H, W, 1.0)
    cur, status, e2 = device_track(ftk, flow, mask, np.empty((B, 0, 2), np.float32), (24, 40))
    assert cur.shape == (B, 0, 2) and status.shape == (B, 0) and e2 is None
    points = point_set(B, H, W, T + 1, (24, 40), 4)
    whole = device_track(ftk, flow, mask, points, (24, 40))
    for b in range(0, B, 2):  # B is just the leading dimension
        part = device_track(ftk, flow[b:b + 2], mask[b:b + 2], points[b:b + 2], (24, 40))
        assert P.same(whole[0][b:b + 2], part[0]) and P.same(whole[1][b:b + 2], part[1])


def test_non_contiguous_points(ftk):
    """The wrapper makes its inputs contiguous first; the device entry refuses them and names the argument."""
    from feature_tracker_amd import device as D
    from feature_tracker_amd import raft
    B, H, W, count = 2, 3, 5, T + 1
    flow, mask, _, _ = fields(5, B, H, W, 1.0)
    points = point_set(B, H, W, count, (24, 40), 6)
    want = P.track(flow, mask, points, (24, 40))
    strided = on_device(np.concatenate([points, points], -1))[:, :, 1:3]  # [B, count, 2] with a row pitch of 4
    strided.copy_(on_device(points))
    assert not strided.is_contiguous()
    got = ftk.track_points_from_flow(on_device(flow), on_device(mask), strided, (24, 40))
    assert P.same(got[0].cpu().numpy(), want[0]) and P.same(got[1].cpu().numpy(), want[1])
    ctx = raft._context(torch.cuda.current_device())
    cur, status = torch.full((B, count, 2), 7.0, device="cuda"), torch.full((B, count), 9, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match=r"^points must be .*pass points\.contiguous\(\)"):
        D.flow_track_points_device(ctx, on_device(flow), on_device(mask), strided, 24, 40, cur, status)
    with pytest.raises(ValueError, match=r"^cur_points must be .*pass cur_points\.contiguous\(\)"):
        D.flow_track_points_device(ctx, on_device(flow), on_device(mask), strided.contiguous(), 24, 40, torch.empty((B, count, 4), device="cuda")[:, :, :2], status)
    torch.cuda.synchronize()
    assert bool((cur == 7.0).all()) and bool((status == 9).all())  # nothing was launched
    D.flow_track_points_device(ctx, on_device(flow), on_device(mask), strided.contiguous(), 24, 40, cur, status)
    assert P.same(cur.cpu().numpy(), want[0]) and P.same(status.cpu().numpy(), want[1])


def test_inference_only_and_native_refusals(ftk):
    import ctypes as C

    from feature_tracker_amd import raft
    B, H, W, count = 1, 2, 3, 5
    flow, mask, _, _ = fields(8, B, H, W, 1.0)
    f, m, p = on_device(flow), on_device(mask), on_device(point_set(B, H, W, count, (16, 24), 1))
    with pytest.raises(RuntimeError, match="inference only"):
        ftk.track_points_from_flow(f.clone().requires_grad_(True), m, p, (16, 24))
    # the C entry itself: every refusal is a recorded error before any launch, and N = 0 is FTK_OK without one
    ctx = raft._context(torch.cuda.current_device())
    cur, status, e2 = torch.full((B, count, 2), 7.0, device="cuda"), torch.full((B, count), 9, dtype=torch.uint8, device="cuda"), torch.full((B, count), 7.0, device="cuda")
    fp, mp, pp, cp, sp, ep = (C.c_void_p(t.data_ptr()) for t in (f, m, p, cur, status, e2))
    inf, nan = float("inf"), float("nan")
    good = dict(flow=fp, mask=mp, flow_back=None, mask_back=None, B=B, H=H, W=W, N=count, rows=16, cols=24, scale=1.0, t=0.0, points=pp, cur=cp, status=sp, e2=ep)
    for change, match in ((dict(flow=None), "null"), (dict(mask=None), "null"), (dict(points=None), "null"), (dict(cur=None), "null"), (dict(status=None), "null"),
                          (dict(B=0), "positive"), (dict(H=-2), "positive"), (dict(W=0), "positive"), (dict(N=-1), "not negative"),
                          (dict(rows=0), "outside"), (dict(rows=17), "outside"), (dict(cols=25), "outside"), (dict(cols=-3), "outside"),
                          (dict(scale=inf), "finite"), (dict(scale=nan), "finite"), (dict(t=-1.0), "negative or NaN"), (dict(t=nan), "negative or NaN"),
                          (dict(flow_back=fp), "half a backward pair"), (dict(mask_back=mp), "half a backward pair"),
                          (dict(H=2 ** 21 + 1, rows=1), "above"), (dict(B=2 ** 31 - 1, H=2 ** 21, W=2 ** 21), "byte count")):
        rc = N.lib().ftk_flow_track_points_device(ctx.handle, None, *{**good, **change}.values())
        assert rc == -1, change
        with pytest.raises(N.FtkError, match=match):
            N.check(rc, ctx.handle)
    assert N.lib().ftk_flow_track_points_device(ctx.handle, None, *{**good, "N": 0}.values()) == 0
    torch.cuda.synchronize()
    assert bool((cur == 7.0).all()) and bool((status == 9).all()) and bool((e2 == 7.0).all())
    assert N.lib().ftk_flow_track_points_device(ctx.handle, None, *{**good, "e2": None}.values()) == 0  # fb_error2 is optional
    torch.cuda.synchronize()
    want = P.track(flow, mask, p.cpu().numpy(), (16, 24))
    assert P.same(cur.cpu().numpy(), want[0]) and P.same(status.cpu().numpy(), want[1]) and bool((e2 == 7.0).all())
    assert N.lib().ftk_flow_track_points_device(ctx.handle, None, *good.values()) == 0  # without a backward pair fb_error2 is all 0
    torch.cuda.synchronize()
    assert bool((e2 == 0).all())


def test_tensors_on_two_devices(ftk):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second HIP device")
    flow, mask, _, _ = fields(9, 1, 2, 3, 1.0)
    points = torch.zeros(1, 4, 2)
    with pytest.raises(ValueError, match="device"):
        ftk.track_points_from_flow(on_device(flow), torch.from_numpy(mask).to("cuda:1"), points.to("cuda:0"), (16, 24))
    with pytest.raises(ValueError, match="points must be on"):
        ftk.track_points_from_flow(on_device(flow), on_device(mask), points.to("cuda:1"), (16, 24))
