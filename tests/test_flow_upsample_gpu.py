"""upsample_flow on the device against the scalar restatement (tests/flow_upsample_ref.c): bit-identical on every shape, logit scale
and mask_scale (any NaN equals any NaN); the torch composition of model.py:48-64 on the same device agrees within
the CPU test's bound, doubled."""
import numpy as np
import pytest

from tests import flow_upsample_ref as R
from tests.test_flow_upsample_cpu import UNITS, hostile_inputs, inputs, torch_upsample

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from feature_tracker_amd import _native as N  # noqa: E402

T = N.FTK_FLOW_UPSAMPLE_TILE
# below one tile in both axes (the first three), around one tile, several tiles with a tail and B > 1, the reference's grid
SHAPES = [(1, 1, 1), (1, 1, 9), (2, 3, 5), (1, 2, T - 1), (1, 2, T), (1, 2, T + 1), (2, 5, 2 * T + 3), (1, 60, 94)]
MASK_SCALES = (1.0, 0.25, 0.3)


def where_differs(got, want):
    return np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5].tolist()


def device_upsample(ftk, flow, mask, mask_scale=1.0):
    dev = torch.device("cuda")
    return ftk.upsample_flow(torch.from_numpy(np.ascontiguousarray(flow)).to(dev), torch.from_numpy(np.ascontiguousarray(mask)).to(dev), mask_scale).cpu().numpy()


@pytest.mark.parametrize("logit_scale", [1.0, 30.0])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_bit_identical_to_the_restatement(ftk, B, H, W, logit_scale):
    """Logit scale 30 puts x - m across exp_c's cutoff and makes near-one-hot weights; mask_scale 0.3 is no power of two, so the
    multiply rounds."""
    flow, mask = inputs(1000 * H + W, B, H, W, logit_scale)
    flow, mask = flow.numpy(), mask.numpy()
    for mask_scale in MASK_SCALES:
        got = device_upsample(ftk, flow, mask, mask_scale)
        want = R.upsample(flow, mask, mask_scale)
        assert got.shape == (B, 2, 8 * H, 8 * W)
        assert R.same(got, want), f"mask_scale {mask_scale}: differs at {where_differs(got, want)}"


def test_hostile_logits(ftk):
    """NaN at k = 0 and at k = 5, +inf, nine -inf, one -inf, x - m on both sides of the cutoff (tests/test_flow_upsample_cpu.py)."""
    flow, mask = hostile_inputs()
    got = device_upsample(ftk, flow, mask)
    want = R.upsample(flow, mask)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert R.same(got, want), where_differs(got, want)


def test_subnormal_products(ftk):
    """Flow values near the bottom of the normal range: 8 * flow * weight is subnormal for most weights, and so are the partial sums."""
    flow, mask = inputs(31, 2, 5, T + 3, 3.0, flow_scale=2e-39)
    flow, mask = flow.numpy().copy(), mask.numpy()
    flow[:, :, :1] *= 1e3  # normal-range neighbours next to subnormal ones
    want = R.upsample(flow, mask)
    tiny = np.finfo(np.float32).tiny
    assert ((np.abs(want) < tiny) & (want != 0)).mean() > 0.3
    got = device_upsample(ftk, flow, mask)
    assert R.same(got, want), where_differs(got, want)


@pytest.mark.parametrize("B,H,W,logit_scale", [(2, 5, 2 * T + 3, 1.0), (1, 60, 94, 1.0), (1, 2, 7, 20.0)])
def test_against_the_torch_composition_on_the_device(ftk, B, H, W, logit_scale):
    dev = torch.device("cuda")
    flow, mask = inputs(41 + W, B, H, W, logit_scale)
    flow, mask = flow.to(dev), mask.to(dev)
    unit = 2.0 ** -24 * float((8 * flow).abs().max())
    for mask_scale in (1.0, 0.25):
        got = ftk.upsample_flow(flow, mask, mask_scale)
        ref = torch_upsample(flow, mask_scale * mask)
        off = float((got - ref).abs().max()) / unit
        print(f"{(B, H, W, logit_scale)}, mask_scale {mask_scale}: {off:.2f} units (bound {2 * UNITS})")
        assert off <= 2 * UNITS


def test_batch_stacking(ftk):
    """B is just the leading dimension: one [3 * 2, ...] call equals three [2, ...] calls."""
    dev = torch.device("cuda")
    flow, mask = inputs(51, 6, 4, T + 5, 2.0)
    flow, mask = flow.to(dev), mask.to(dev)
    whole = ftk.upsample_flow(flow, mask, 0.25).cpu().numpy()
    for n in range(3):
        part = ftk.upsample_flow(flow[2 * n:2 * n + 2], mask[2 * n:2 * n + 2], 0.25).cpu().numpy()
        assert R.same(whole[2 * n:2 * n + 2], part), n


def test_graph_capture_and_two_replays(ftk):
    """One call recorded in torch.cuda.graph on a single stream, replayed twice with the inputs overwritten in place in between:
    each replay equals the eager result on the same inputs bit for bit."""
    dev = torch.device("cuda")
    sets = [tuple(t.to(dev) for t in inputs(61 + n, 2, 6, T + 9, 3.0)) for n in range(3)]
    eager = [ftk.upsample_flow(f, m, 0.3).cpu().numpy() for f, m in sets]
    flow, mask = sets[0][0].clone(), sets[0][1].clone()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ftk.upsample_flow(flow, mask, 0.3)  # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ftk.upsample_flow(flow, mask, 0.3)
    for n in (1, 2):
        flow.copy_(sets[n][0])
        mask.copy_(sets[n][1])
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert R.same(out.cpu().numpy(), eager[n]), f"replay {n}"


def test_non_contiguous_inputs(ftk):
    """The wrapper makes its inputs contiguous first; the device entry refuses them and names the argument."""
    from feature_tracker_amd import device as D
    from feature_tracker_amd import raft
    dev = torch.device("cuda")
    flow, mask = inputs(71, 1, 4, 6, 1.0)
    flow_t = flow.to(dev).transpose(2, 3).contiguous().transpose(2, 3)  # [1, 2, 4, 6] with strides of [1, 2, 6, 4]
    mask_t = mask.to(dev).transpose(2, 3).contiguous().transpose(2, 3)
    assert not flow_t.is_contiguous() and not mask_t.is_contiguous()
    want = R.upsample(flow.numpy(), mask.numpy())
    assert R.same(ftk.upsample_flow(flow_t, mask_t).cpu().numpy(), want)
    ctx = raft._context(torch.cuda.current_device())
    out = torch.full((1, 2, 32, 48), 7.0, device=dev)
    with pytest.raises(ValueError, match=r"^flow must be .*pass flow\.contiguous\(\)"):
        D.flow_upsample_device(ctx, flow_t, mask_t.contiguous(), out)
    with pytest.raises(ValueError, match=r"^mask must be .*pass mask\.contiguous\(\)"):
        D.flow_upsample_device(ctx, flow_t.contiguous(), mask_t, out)
    with pytest.raises(ValueError, match=r"^out must be .*pass out\.contiguous\(\)"):
        D.flow_upsample_device(ctx, flow_t.contiguous(), mask_t.contiguous(), torch.empty((1, 2, 48, 32), device=dev).transpose(2, 3))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
    D.flow_upsample_device(ctx, flow_t.contiguous(), mask_t.contiguous(), out)
    assert R.same(out.cpu().numpy(), want)


def test_inference_only_and_native_refusals(ftk):
    from feature_tracker_amd import raft
    dev = torch.device("cuda")
    flow, mask = inputs(81, 1, 2, 3, 1.0)
    flow, mask = flow.to(dev), mask.to(dev)
    g = flow.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        ftk.upsample_flow(g, mask)
    with torch.no_grad():
        assert R.same(ftk.upsample_flow(g, mask).cpu().numpy(), ftk.upsample_flow(flow, mask).cpu().numpy())
    # the C entry itself: non-positive sizes, null pointers and a non-finite scale are recorded errors, before any launch
    import ctypes as C
    ctx = raft._context(torch.cuda.current_device())
    out = torch.full((1, 2, 16, 24), 7.0, device=dev)
    f, m, o = (C.c_void_p(t.data_ptr()) for t in (flow, mask, out))
    for args, match in (((f, m, 0, 2, 3, 1.0, o), "positive"), ((f, m, 1, 2, -3, 1.0, o), "positive"), ((None, m, 1, 2, 3, 1.0, o), "null"),
                        ((f, m, 1, 2, 3, 1.0, None), "null"), ((f, m, 1, 2, 3, float("inf"), o), "finite"), ((f, m, 1, 2, 3, float("nan"), o), "finite")):
        rc = N.lib().ftk_flow_upsample_device(ctx.handle, None, *args)
        assert rc == -1
        with pytest.raises(N.FtkError, match=match):
            N.check(rc, ctx.handle)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_tensors_on_two_devices(ftk):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second HIP device")
    flow, mask = inputs(91, 1, 2, 3, 1.0)
    with pytest.raises(ValueError, match="device"):
        ftk.upsample_flow(flow.to("cuda:0"), mask.to("cuda:1"))
