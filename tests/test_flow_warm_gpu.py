"""warm_start_flow on the device: bit-identical to the scalar restatement (tests/flow_warm_ref.c) at every shape where the
kernel takes another path — one pixel, one row, one column, below and above a tile of FTK_FLOW_WARM_TILE = 256 targets and sources, and
33 x 65 = 2 145 pixels: nine tiles of targets, nine LDS tiles of sources, and nine splits by the automatic rule — in the one-launch form,
the automatic form and forced split counts; what the call leaves alone; a repeated call; graph capture; and the loud failures."""
import functools

import numpy as np
import pytest

from tests import flow_warm_ref as R
from tests.test_flow_warm_cpu import gaussian_flow, integer_flow

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN, INF = float("nan"), float("inf")
SHAPES = [(1, 1), (1, 70), (70, 1), (8, 8), (9, 17), (33, 65)]
KINDS = ["sigma 2", "sigma 40", "integers", "hostile"]


def flows_of(kind, B, H, W, seed):
    if kind == "integers":
        return integer_flow(B, H, W, seed)
    if kind == "sigma 40":
        return gaussian_flow(B, H, W, 40.0, seed)
    flow = gaussian_flow(B, H, W, 2.0, seed)
    if kind == "hostile":  # NaN, +-inf and a huge value sprinkled in, about one pixel in eight
        rng = np.random.default_rng(seed + 1)
        where = rng.uniform(size=flow.shape) < 0.06
        flow[where] = rng.choice(np.float32([NAN, INF, -INF, 1e30, -1e30]), size=int(where.sum()))
    return flow


@functools.lru_cache(maxsize=None)
def case(kind, shape, B):
    """(flow, the restatement's output): a different flow per entry; at B 3 entry 1 has no valid source and entry 2 is zero."""
    H, W = shape
    flow = flows_of(kind, B, H, W, 10 * H + W)
    if B == 3:
        flow[1] = np.float32(-2.0 * max(H, W))
        flow[2] = 0.0
    want = R.warm(flow)
    flow.setflags(write=False)
    want.setflags(write=False)
    return flow, want


def on_device(a):
    return torch.from_numpy(np.array(a, copy=True)).to("cuda")  # a copy: the cases are read-only


def forced(ftk, flow, splits):
    """device.flow_warm_device with a split count of the caller's and a workspace full of ones, which the call must not depend on."""
    from feature_tracker_amd import device as D
    from feature_tracker_amd import raft
    out = torch.full_like(flow, NAN)
    B, _, H, W = flow.shape
    workspace = torch.full((splits * B * H * W,), -1, dtype=torch.int64, device=flow.device) if splits > 1 else None
    D.flow_warm_device(raft._device_context(flow), flow, out, splits, workspace)
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("kind", KINDS)
def test_bit_identical_to_the_restatement(ftk, kind, shape, B):
    from feature_tracker_amd import _native as N
    flow, want = case(kind, shape, B)
    d_flow = on_device(flow)
    got = ftk.warm_start_flow(d_flow)
    assert got.shape == d_flow.shape and got.dtype == torch.float32 and got.data_ptr() != d_flow.data_ptr()
    assert R.same(got.cpu().numpy(), want)
    assert R.same(d_flow.cpu().numpy(), flow)  # the input is left alone
    if B == 3:
        assert got[1].cpu().numpy().view(np.uint32).max() == 0  # no valid source: +0
    auto = N.flow_warm_splits(B, *shape)
    for splits in sorted({1, 2, 5, N.FTK_FLOW_WARM_MAX_SPLITS} - {auto}):  # 5 and 32 are more splits than tiles at the small shapes: empty ranges
        assert R.same(forced(ftk, d_flow, splits).cpu().numpy(), want), splits


def test_the_shapes_cover_the_paths():
    from feature_tracker_amd import _native as N
    T = N.FTK_FLOW_WARM_TILE
    assert 33 * 65 > 2 * T and N.flow_warm_splits(1, 33, 65) >= 2 and N.flow_warm_splits(3, 33, 65) >= 2  # tiles of targets, LDS tiles, splits
    assert N.flow_warm_splits(1, 8, 8) == 1 and 70 < T < 9 * 17 + T  # the one-launch form by the automatic rule, and a tile's edge
    flow, want = case("integers", (9, 17), 1)
    _, chosen = R.warm(flow, with_chosen=True)
    _, highest = R.warm(flow, R.MUTANT_HIGHEST_INDEX, with_chosen=True)
    assert (chosen != highest).mean() > 0.2  # ties are everywhere in the whole-number flows: the tie-break is what they test
    hostile, _ = case("hostile", (33, 65), 1)
    assert np.isnan(hostile).any() and np.isinf(hostile).any() and (np.abs(hostile[np.isfinite(hostile)]) > 1e29).any()


def test_a_second_call_gives_the_same_bits(ftk):
    """Nothing is left over from a call: the same input again, after a call on another input of the same shape, gives the same bits."""
    flow, want = case("sigma 2", (33, 65), 3)
    other, other_want = case("integers", (33, 65), 3)
    d_flow, d_other = on_device(flow), on_device(other)
    first = ftk.warm_start_flow(d_flow)
    between = ftk.warm_start_flow(d_other)
    second = ftk.warm_start_flow(d_flow)
    assert second.data_ptr() != first.data_ptr()
    assert R.same(first.cpu().numpy(), want) and R.same(second.cpu().numpy(), want) and R.same(between.cpu().numpy(), other_want)


@pytest.mark.parametrize("shape", [(8, 8), (33, 65)], ids=["one launch", "two launches"])
def test_graph_capture_and_replay_on_a_changed_input(ftk, shape):
    flow, _ = case("sigma 2", shape, 3)
    other, other_want = case("hostile", shape, 3)
    held = on_device(flow)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ftk.warm_start_flow(held)  # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ftk.warm_start_flow(held)
    held.copy_(on_device(other))
    out.fill_(NAN)
    g.replay()
    torch.cuda.synchronize()
    assert R.same(out.cpu().numpy(), other_want)
    assert R.same(ftk.warm_start_flow(held).cpu().numpy(), other_want)


def test_argument_errors_launch_nothing(ftk, monkeypatch):
    """Every refusal of tests/test_flow_warm_args_cpu.py with tensors on the device: a ValueError, and the library is not entered."""
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    from feature_tracker_amd import raft
    good = torch.zeros(2, 2, 3, 5, device="cuda")
    ctx = raft._device_context(good)
    N.lib()
    entered = []

    class Telltale:
        def __getattr__(self, name):
            entered.append(name)
            raise AssertionError(f"{name} was reached")

    monkeypatch.setattr(N, "lib", lambda: Telltale())
    for match, bad in (("flow must be", good.double()), ("flow must be", good.half()), ("flow must be", good[0]), ("flow must be", torch.zeros(2, 3, 3, 5, device="cuda")),
                       ("must not be empty", torch.zeros(2, 2, 0, 5, device="cuda")), ("contiguous", torch.zeros(2, 2, 5, 3, device="cuda").transpose(2, 3)),
                       ("FTK_FLOW_WARM_MAX_PIXELS", torch.zeros(1, 2, 1025, 1024, device="cuda")), ("no CPU fallback", good.cpu())):
        with pytest.raises(ValueError, match=match):
            ftk.warm_start_flow(bad)
    with pytest.raises(RuntimeError, match="inference only"):
        ftk.warm_start_flow(good.clone().requires_grad_(True))
    out, words = torch.zeros_like(good), torch.zeros(2 * 2 * 3 * 5, dtype=torch.int64, device="cuda")
    for match, args in (("out must be", (good, out[:1])), ("out must be", (good, out.double())), ("out must be", (good, out.cpu())),
                        ("flow must be.*strided view", (good.transpose(2, 3), out)), ("splits must be", (good, out, 33, words)),
                        ("go together", (good, out, 2)), ("workspace must be.*too few", (good, out, 3, words)),
                        ("workspace must be.*wrong dtype", (good, out, 2, words.to(torch.int32)))):
        with pytest.raises(ValueError, match=match):
            D.flow_warm_device(ctx, *args)
    assert entered == []


def test_native_refusals_launch_nothing(ftk):
    import ctypes as C

    from feature_tracker_amd import _native as N
    from feature_tracker_amd import raft
    flow = torch.zeros(1, 2, 3, 5, device="cuda")
    out, words = torch.full_like(flow, 7.0), torch.zeros(64, dtype=torch.int64, device="cuda")
    ctx = raft._device_context(flow)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    entry = N.lib().ftk_flow_warm_device
    for args in ((None, 1, 3, 5, 1, None, p(out)), (p(flow), 1, 3, 5, 1, None, None), (p(flow), 1, 3, 5, 1, None, p(flow)), (p(flow), 0, 3, 5, 1, None, p(out)),
                 (p(flow), 1, 0, 5, 1, None, p(out)), (p(flow), 1, 1025, 1024, 1, None, p(out)), (p(flow), 1, 3, 5, 0, None, p(out)),
                 (p(flow), 1, 3, 5, 33, p(words), p(out)), (p(flow), 1, 3, 5, 2, None, p(out))):
        assert entry(ctx.handle, stream, *args) == -1, args
    torch.cuda.synchronize()
    assert (out == 7.0).all()
