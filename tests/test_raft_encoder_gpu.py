"""The strided conv2d_kernel forms, FeatureEncoder, ContextEncoder and Raft on the device against the scalar restatement
(tests/raft_encoder_ref.c and the networks tests/raft_encoder_ref.py composes): bit-identical on every shape, channel count, stride and
epilogue (any NaN equals any NaN), and within the CPU test's bounds of the float64 composition evaluated on the CPU.  The
layer shapes are the smallest that reach each edge of a tile of 32 output channels x 32 output pixels x wn rows (wn = 4, 2, 1 for 1, 2,
>= 3 tiles of output channels), of a chunk of 32 / 8 input channels, and of the even / odd staging planes of stride 2."""
import functools

import numpy as np
import pytest

from tests import raft_encoder_ref as E
from tests.test_raft_encoder_cpu import (ENCODER_BOUND, ENCODER_CASES, RAFT_BOUND, RAFT_CASES, encoder_case, encoder_restated, make_image, max_abs,
                                         raft_case, raft_restated)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WIDTHS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 129)
HEIGHTS = (1, 2, 3, 4, 5, 8, 9)
# (kernel_size, C_in): a partial last chunk of 8 / 32 input channels
KERNELS = ((3, 9), (1, 33))
C_OUTS = (2, 33, 40, 100)  # wm 1, 2, 2, 4


def where_differs(got, want):
    return np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5].tolist()


def on_device(t):
    return torch.from_numpy(np.ascontiguousarray(t)).to("cuda")


def make_layer(Cin, Cout, ks, stride, B, H, W, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, ks, ks)) / np.sqrt(Cin * ks * ks)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    res = rng.standard_normal((B, Cout, -(-H // stride), -(-W // stride))).astype(np.float32)
    return x, w, b, res


def run_layer(x, weight, bias, stride, residual, relu, scale=1.0, normalise=False):
    """conv2d_strided_device on numpy operands; also asserts that the call left its inputs and the residual as they were."""
    from feature_tracker_amd import device as D
    from feature_tracker_amd import raft
    dx, dres = on_device(x), None if residual is None else on_device(residual)
    B, _, H, W = x.shape
    out = torch.full((B, weight.shape[0], -(-H // stride), -(-W // stride)), float("nan"), device="cuda")
    ctx = raft._context(torch.cuda.current_device())
    D.conv2d_strided_device(ctx, [dx], raft._pack_conv(on_device(weight)), on_device(bias), weight.shape[2], stride, relu, scale, dres, normalise, out)
    assert E.same(dx.cpu().numpy(), x) and (residual is None or E.same(dres.cpu().numpy(), residual))
    return out.cpu().numpy()


@pytest.mark.parametrize("ks,Cin", KERNELS, ids=["3x3", "1x1"])
@pytest.mark.parametrize("Cout", C_OUTS)
def test_stride_2_bit_identical_to_the_restatement(ftk, ks, Cin, Cout):
    """Every width and height of the lists (B 2), the four epilogues (residual x ReLU) dealt over them so that each occurs at every wn."""
    for n, (H, W) in enumerate([(h, WIDTHS[(i * 3 + 1) % len(WIDTHS)]) for i, h in enumerate(HEIGHTS)] + [(HEIGHTS[(i * 2) % len(HEIGHTS)], w)
                                                                                                            for i, w in enumerate(WIDTHS)]):
        x, w, b, res = make_layer(Cin, Cout, ks, 2, 2, H, W, 100 + n)
        for with_res, relu in ((n % 2 == 0, n % 4 < 2), (n % 2 == 1, n % 4 >= 2)):
            got = run_layer(x, w, b, 2, res if with_res else None, relu)
            want = E.conv2d(x, w, b, 2, res if with_res else None, relu)
            assert got.shape == want.shape == (2, Cout, -(-H // 2), -(-W // 2))
            assert E.same(got, want), f"H {H} W {W} residual {with_res} relu {relu}: differs at {where_differs(got, want)}"


@pytest.mark.parametrize("ks,Cin,Cout,H,W", [(3, 9, 33, 5, 35), (1, 33, 100, 9, 67), (3, 9, 2, 9, 33), (7, 3, 40, 5, 35)])
def test_stride_1_with_residual_and_normalisation(ftk, ks, Cin, Cout, H, W):
    x, w, b, res = make_layer(Cin, Cout, ks, 1, 2, H, W, 7)
    for relu in (True, False):
        got, want = run_layer(x, w, b, 1, res, relu), E.conv2d(x, w, b, 1, res, relu)
        assert E.same(got, want), where_differs(got, want)
    pixels = np.floor(np.abs(x) * 100) % 256
    got, want = run_layer(pixels, w, b, 1, None, True, normalise=True), E.conv2d(pixels, w, b, 1, None, True, normalise=True)
    assert E.same(got, want), where_differs(got, want)
    plain = run_layer(x, w, b, 1, None, True, 0.25)  # nothing of the extension asked for: the plain form
    assert E.same(plain, E.conv2d(x, w, b, 1, None, True, 0.25))


@pytest.mark.parametrize("ks,Cin", KERNELS, ids=["3x3", "1x1"])
def test_hostile_values(ftk, ks, Cin):
    """NaN, +-inf, -0 and subnormals in the input and in the residual, and a residual that meets an accumulator of the other sign."""
    x, w, b, res = make_layer(Cin, 40, ks, 2, 2, 9, 66, 8)
    hostile = np.float32([np.nan, np.inf, -np.inf, -0.0, 1e-40, -3e-39, 0.0])
    x.reshape(-1)[::97][:70] = np.tile(hostile, 10)
    res.reshape(-1)[::53][:70] = np.tile(hostile, 10)
    b[::3] = -0.0
    for relu in (True, False):
        got, want = run_layer(x, w, b, 2, res, relu), E.conv2d(x, w, b, 2, res, relu)
        assert np.isnan(want).any() and not np.isnan(want).all()
        assert E.same(got, want), where_differs(got, want)
    # relu(acc + res) keeps a NaN and -0: a one-tap layer whose accumulator is exactly the input
    x = np.float32([-0.0, np.nan, -3.0, np.inf, 5.0, 0.0, 1e-40]).reshape(1, 1, 1, 7)
    one = np.ones((1, 1, 1, 1), np.float32)
    res = np.float32([-0.0, 1.0, 1.0, -np.inf, -5.0, -0.0, -1e-40, 0.0]).reshape(1, 1, 1, 8)[:, :, :, :4]
    got, want = run_layer(x, one, np.float32([-0.0]), 2, res, True), E.conv2d(x, one, np.float32([-0.0]), 2, res, True)
    assert E.same(got, want), (got, want)
    assert np.signbit(want[0, 0, 0, 0]) and want[0, 0, 0, 0] == 0


# ---- whole encoders and the model ---------------------------------------------------------------------------------------------------


def device_state(state):
    return {k: torch.from_numpy(np.asarray(v)).to("cuda") for k, v in state.items()}


@pytest.mark.parametrize("k", range(len(ENCODER_CASES)), ids=[str(c) for c in ENCODER_CASES])
def test_encoders_bit_identical_and_within_the_bound_of_float64(ftk, k):
    state, image, ref64 = encoder_case(k, 1)
    want = encoder_restated(k, 1)
    enc = ftk.FeatureEncoder.from_state_dict(device_state(state))
    got = enc(on_device(image), normalise=True)
    assert got.is_contiguous() and E.same(got.cpu().numpy(), want), where_differs(got.cpu().numpy(), want)
    print(f"FeatureEncoder {ENCODER_CASES[k]} vs float64: {max_abs(got.cpu().numpy(), ref64):.3g} (bound {ENCODER_BOUND:.3g})")
    assert max_abs(got.cpu().numpy(), ref64) <= ENCODER_BOUND
    plain = enc(on_device(E.normalise(image)))  # the normalisation at the fetch is the normalisation before it
    assert E.same(plain.cpu().numpy(), want)
    # the same weights as a ContextEncoder, split at an odd channel
    M = ENCODER_CASES[k][0]
    split = M // 2 - 1
    ctx_enc = ftk.ContextEncoder.from_state_dict(device_state({"net." + key: v for key, v in state.items()}), context_channels=split)
    inp, net = ctx_enc(on_device(image), normalise=True)
    assert inp.is_contiguous() and net.is_contiguous() and (inp.shape[1], net.shape[1]) == (split, M - split)
    assert E.same(inp.cpu().numpy(), want[:, :split]) and E.same(net.cpu().numpy(), want[:, split:])


@functools.lru_cache(maxsize=None)
def device_raft(ftk, k):
    c = RAFT_CASES[k]
    state, ref_image, cur_image, ref64 = raft_case(k, 1)
    model = ftk.Raft.from_state_dict(device_state(state), c[3], c[4], max_iterations=c[14])
    return model, on_device(ref_image), on_device(cur_image), raft_restated(k, 1), ref64


@pytest.mark.parametrize("k", range(len(RAFT_CASES)), ids=[str(c) for c in RAFT_CASES])
def test_raft_bit_identical_and_within_the_bound_of_float64(ftk, k):
    model, ref_image, cur_image, want, ref64 = device_raft(ftk, k)
    got = [p.cpu().numpy() for p in model(ref_image, cur_image)]
    assert len(got) == len(want) == RAFT_CASES[k][14]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and E.same(g, w), f"prediction {i} differs at {where_differs(g, w)}"
    print(f"Raft {RAFT_CASES[k]} vs float64: {max_abs(got, ref64):.3g} (bound {RAFT_BOUND:.3g})")
    assert max_abs(got, ref64) <= RAFT_BOUND
    assert len(model(ref_image, cur_image, iterations=1)) == 1


def test_graph_capture_and_replay(ftk):
    """The whole forward recorded in torch.cuda.graph on a single stream, replayed twice with the images overwritten in place."""
    k = 1
    c = RAFT_CASES[k]
    model, ref_image, cur_image, want, _ = device_raft(ftk, k)
    B, H, W = c[11:14]
    other = [on_device(make_image(B, 1, H, W, 90 + n).numpy()) for n in range(2)]
    eager_other = [p.cpu().numpy() for p in model(*other)]
    held = [ref_image.clone(), cur_image.clone()]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        model(*held)  # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = model(*held)
    for images, expect in ((other, eager_other), ((ref_image, cur_image), want)):
        for h, s in zip(held, images):
            h.copy_(s)
        for o in out:
            o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for i, (o, e) in enumerate(zip(out, expect)):
            assert E.same(o.cpu().numpy(), e), i


def test_native_refusals_launch_nothing(ftk):
    import ctypes as C

    from feature_tracker_amd import _native as N
    from feature_tracker_amd import raft
    ctx = raft._context(torch.cuda.current_device())
    x = torch.zeros(1, 8, 5, 6, device="cuda")
    out = torch.full((1, 8, 3, 3), 7.0, device="cuda")
    w, b = torch.zeros(N.conv2d_packed_elements(8, 8, 7), device="cuda"), torch.zeros(8, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    part = (N.GruPart * 1)(N.GruPart(ptr(x), 8))
    for ks, stride, match in ((7, 2, "stride 2 with kernel_size 7"), (3, 3, "stride 3"), (3, 0, "stride 0"), (5, 2, "kernel_size 5")):
        rc = N.lib().ftk_conv2d_strided_device(ctx.handle, None, part, 1, ptr(w), ptr(b), 8, ks, stride, 1, 1.0, None, 0, 1, 5, 6, ptr(out))
        assert rc == -4
        with pytest.raises(N.FtkError, match=match):
            N.check(rc, ctx.handle)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
