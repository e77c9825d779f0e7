"""SuperPoint on the device against the scalar restatement (tests/superpoint_ref.c), bit for bit (any NaN equal to any
NaN): conv2d_kernel's pooled form over tests/test_superpoint_cpu.py's cases and a hostile image, the normalise kernel at the tile and
vector edges with a zero and a NaN cell, the whole network at narrow and at upstream's widths, ``detect`` against ``KeypointDecoder`` on
the restatement's heads, the stacked head layer against two launches, one pass replayed from a captured graph, and the refusals of the
library."""
import numpy as np
import pytest

from tests import keypoint_decode_ref as K
from tests import superpoint_ref as R
from tests import test_superpoint_cpu as T

pytestmark = pytest.mark.gpu


def _ctx(t):
    from feature_tracker_amd.raft import _device_context
    return _device_context(t)


def _pool_on_device(parts, weight, bias, relu):
    import torch
    from feature_tracker_amd import device as D
    from feature_tracker_amd import raft
    d_parts = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in parts]
    B, _, H, W = d_parts[0].shape
    M, ks = weight.shape[0], weight.shape[-1]
    out = torch.full((B, M, H // 2, W // 2), 7.0, device="cuda")
    D.conv2d_pool_device(_ctx(out), d_parts, raft._pack_conv(torch.from_numpy(np.ascontiguousarray(weight)).cuda()),
                         torch.from_numpy(np.ascontiguousarray(bias)).cuda(), ks, relu, out)
    torch.cuda.synchronize()
    assert all(R.same(d.cpu().numpy(), p) for d, p in zip(d_parts, parts))  # the inputs are left untouched
    return out.cpu().numpy()


@pytest.mark.parametrize("k", range(len(T.POOL_CASES)), ids=[str(c) for c in T.POOL_CASES])
def test_pooled_layer_is_the_restatement(ftk, k):
    relu = T.POOL_CASES[k][1]
    parts, weight, bias = T.pool_case(k)
    assert R.same(_pool_on_device(parts, weight, bias, relu), R.conv2d_pool(parts, weight, bias, relu))


@pytest.mark.parametrize("relu", [False, True])
def test_pooled_layer_on_hostile_values(ftk, relu):
    x, weight, bias = T.hostile_pool_layer()
    want = R.conv2d_pool(x, weight, bias, relu)
    assert np.isnan(want).any() and np.isinf(want).any() and (np.signbit(want) & (want == 0)).any()
    assert R.same(_pool_on_device([x], weight, bias, relu), want)


@pytest.mark.parametrize("d", T.NORMALISE_CHANNELS)
@pytest.mark.parametrize("grid", T.NORMALISE_GRIDS, ids=str)
def test_normalise_kernel_is_the_restatement(ftk, d, grid):
    import torch
    from feature_tracker_amd import device as D
    cases = [T.normalise_case(d, *grid)]
    if grid == (1, 1):  # no room for the special cells in the case itself
        cases += [np.zeros((d, 1, 1), np.float32), np.full((d, 1, 1), np.nan, np.float32)]
    for x in cases:
        d_x = torch.from_numpy(x.copy()).cuda()
        y = torch.full(grid + (d,), 7.0, device="cuda")
        D.channel_normalise_device(_ctx(y), d_x, y)
        torch.cuda.synchronize()
        assert R.same(y.cpu().numpy(), R.channel_normalise(x)) and R.same(d_x.cpu().numpy(), x)
    # the returned view is one KeypointDecoder.decode takes, and gives the bits of the contiguous layout
    if grid != (1, 1):
        semi, _ = K.heads(grid[0], grid[1], d, 5)
        y.copy_(torch.from_numpy(np.nan_to_num(R.channel_normalise(x))))
        decoder = ftk.KeypointDecoder(max_keypoints=16, min_score=0.05, min_distance=4, border=0)
        d_semi = torch.from_numpy(semi.copy()).cuda()
        a, b = decoder.decode(d_semi, y.permute(2, 0, 1)), decoder.decode(d_semi, y.permute(2, 0, 1).contiguous())
        torch.cuda.synchronize()
        assert int(a.count.item()) == int(b.count.item()) > 0 and R.same(a.descriptors.cpu().numpy(), b.descriptors.cpu().numpy())


def _network(ftk, k, seed=T.MEASURED_SEEDS[0]):
    import torch
    widths, H, W = T.NETWORK_CASES[k]
    state, image = T.network_case(k, seed)
    sp = ftk.SuperPoint.from_state_dict({name: torch.from_numpy(v.copy()).cuda() for name, v in state.items()})
    return sp, state, image, torch.from_numpy(image.copy()).cuda()


@pytest.mark.parametrize("k", range(len(T.NETWORK_CASES)), ids=[str(c) for c in T.NETWORK_CASES])
def test_network_heads_and_detect_are_the_restatement(ftk, k):
    import torch
    sp, state, image, d_image = _network(ftk, k)
    want_semi, want_desc = T.network_heads(k, T.MEASURED_SEEDS[0])
    semi, desc = sp.heads(d_image)
    torch.cuda.synchronize()
    assert tuple(semi.shape) == want_semi.shape and tuple(desc.shape) == want_desc.shape and desc.permute(1, 2, 0).is_contiguous()
    assert R.same(semi.cpu().numpy(), want_semi) and R.same(desc.cpu().numpy(), want_desc)
    assert R.same(d_image.cpu().numpy(), image)
    # [1, 1, H, W] is the same call
    semi4, desc4 = sp.heads(d_image[None, None])
    assert semi4.data_ptr() == semi.data_ptr() and R.same(semi4.cpu().numpy(), want_semi) and R.same(desc4.cpu().numpy(), want_desc)
    # detect: the decoder on these heads, against the decoder's restatement on the network's
    kw = dict(min_score=0.0, min_distance=2, border=0)  # seeded weights: every score is near 1 / 65, so no threshold
    decoder = ftk.KeypointDecoder(max_keypoints=64, **kw)
    got = sp.detect(d_image, decoder, return_heatmap=True)
    torch.cuda.synchronize()
    want = K.decode(want_semi, np.ascontiguousarray(want_desc), max_keypoints=64, **kw)
    r = K.Result()
    r.uv, r.scores, r.descriptors, r.count, r.heatmap = (got.uv.cpu().numpy(), got.scores.cpu().numpy(), got.descriptors.cpu().numpy(), int(got.count.item()),
                                                         got.heatmap.cpu().numpy())
    assert want.count > 0 and K.same_results(r, want) == []


def test_stacked_head_layer_is_two_launches(ftk):
    import torch
    from feature_tracker_amd import device as D
    from feature_tracker_amd import raft
    sp, state, image, d_image = _network(ftk, 1)
    sp.heads(d_image)
    bufs = sp._buffers[(d_image.device, 16, 24)]
    x = bufs["conv4b"]
    for name, got in (("convPa", bufs["convPa"]), ("convDa", bufs["convDa"])):
        w = torch.from_numpy(state[name + ".weight"].copy()).cuda()
        out = torch.empty((1, w.shape[0]) + tuple(x.shape[2:]), device="cuda")
        D.conv2d_device(_ctx(x), [x], raft._pack_conv(w), torch.from_numpy(state[name + ".bias"].copy()).cuda(), 3, True, 1.0, out)
        torch.cuda.synchronize()
        assert R.same(out.cpu().numpy(), got.cpu().numpy()), name


def test_a_captured_pass_replayed_on_another_image_equals_the_eager_result(ftk):
    import torch
    sp, state, image, d_image = _network(ftk, 2)
    sp.heads(d_image)  # the buffers of this size are made here, outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        semi, desc = sp.heads(d_image)
    image2 = R.make_image(40, 72, 9)
    d_image.copy_(torch.from_numpy(image2))
    graph.replay()
    torch.cuda.synchronize()
    got = semi.cpu().numpy().copy(), desc.cpu().numpy().copy()
    eager = sp.heads(torch.from_numpy(image2.copy()).cuda())
    torch.cuda.synchronize()
    assert R.same(got[0], eager[0].cpu().numpy()) and R.same(got[1], eager[1].cpu().numpy())
    want = R.heads(image2, state)
    assert R.same(got[0], want[0]) and R.same(got[1], want[1])


def test_the_context_stream_and_the_refusals_of_the_library(ftk):
    import ctypes as C
    import torch
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    ctx = D.context_on_stream(torch.cuda.Stream())
    state, image = T.network_case(1, T.MEASURED_SEEDS[0])
    sp = ftk.SuperPoint.from_state_dict({name: torch.from_numpy(v.copy()).cuda() for name, v in state.items()}, ctx=ctx)
    semi, desc = sp.heads(torch.from_numpy(image.copy()).cuda())
    torch.cuda.synchronize()
    want = T.network_heads(1, T.MEASURED_SEEDS[0])
    assert R.same(semi.cpu().numpy(), want[0]) and R.same(desc.cpu().numpy(), want[1])
    x, w, b = torch.zeros(1, 3, 4, 6, device="cuda"), torch.zeros(N.conv2d_packed_elements(4, 3, 7), device="cuda"), torch.zeros(4, device="cuda")
    out = torch.full((1, 4, 2, 3), 7.0, device="cuda")
    part = lambda: N.part_array([x])  # noqa: E731

    def pool(ks=3, H=4, W=6, o=out.data_ptr(), n_parts=1, M=4):
        return N.lib().ftk_conv2d_pool_device(ctx.handle, None, part(), n_parts, C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()), M, ks, 1, 1, H, W,
                                              None if o is None else C.c_void_p(o))

    assert pool(ks=7) == -4 and pool(ks=5) == -4 and pool(M=1025) == -4  # FTK_E_UNSUPPORTED
    assert pool(H=1) in (-1, -4) and pool(W=1) in (-1, -4) and pool(o=None) == -1 and pool(n_parts=0) == -1 and pool(H=0) == -1  # FTK_E_INVALID_ARGUMENT
    y = torch.full((2, 3, 8), 7.0, device="cuda")
    norm = lambda d=8, hc=2, wc=3, o=y.data_ptr(): N.lib().ftk_channel_normalise_device(  # noqa: E731
        ctx.handle, None, C.c_void_p(x.data_ptr()), d, hc, wc, None if o is None else C.c_void_p(o))
    assert norm(d=0) == -1 and norm(d=1025) == -1 and norm(hc=0) == -1 and norm(wc=-1) == -1 and norm(o=None) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all().item() and (y == 7.0).all().item()  # nothing was launched
