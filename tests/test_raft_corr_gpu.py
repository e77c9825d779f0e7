"""CorrelationPyramid on the device against the scalar restatement (tests/raft_corr_ref.c): every level of the volume and every
lookup is bit-identical (any NaN equals any NaN); the torch-GPU composition of the reference agrees within the CPU
test's bounds."""
import numpy as np
import pytest

from tests import raft_corr_ref as R
from tests.test_raft_corr_cpu import LEVEL0_REL_TOL, LOOKUP_TOL, torch_lookup, torch_pyramid

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def features(seed, B, C, H, W, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, C, H, W, generator=g) * scale).float(), (torch.randn(B, C, H, W, generator=g) * scale).float()


def coords_for(seed, B, H, W, spread=1.4, shift=-3.0):
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([W, H], dtype=torch.float32).view(1, 2, 1, 1)
    return (torch.rand(B, 2, H, W, generator=g) * scale * spread + shift).float()


def check(ftk, f0, f1, L, r, coords):
    """Device pyramid + both lookup forms against the restatement, bit for bit; returns the device object."""
    dev = torch.device("cuda")
    cp = ftk.CorrelationPyramid(f0.to(dev), f1.to(dev), L, r)
    want = R.build(f0.numpy(), f1.numpy(), L)
    assert len(cp.correlation_pyramid) == L
    for l, (got, w) in enumerate(zip(cp.correlation_pyramid, want)):
        g = got[:, 0].cpu().numpy()
        assert R.same(g, w), f"level {l} differs at {np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:5].tolist()}"
    want_out = R.lookup(want, coords.numpy(), r)
    fused = cp.lookup(coords.to(dev)).cpu().numpy()
    assert R.same(fused, want_out), f"lookup differs at {np.argwhere(fused.view(np.uint32) != want_out.view(np.uint32))[:5].tolist()}"
    per_level = cp(coords.to(dev))
    K = (2 * r + 1) ** 2
    for l, t in enumerate(per_level):
        assert t.is_contiguous() and tuple(t.shape) == (f0.shape[0], f0.shape[2], f0.shape[3], K)
        assert R.same(t.cpu().numpy(), np.moveaxis(want_out[:, l * K:(l + 1) * K], 1, -1))
    return cp


def test_reference_main_shape(ftk):
    """correlation_volumes.py's __main__: B 5, C 128, 8 x 8, 3 levels, r 3."""
    f0, f1 = features(1, 5, 128, 8, 8)
    check(ftk, f0, f1, 3, 3, coords_for(2, 5, 8, 8))


@pytest.mark.parametrize("C,L,r", [(128, 3, 3), (256, 4, 4)])
def test_eighth_of_the_example_pair(ftk, C, L, r):
    """1/8 of the reference's example pair (752 x 480 -> 94 x 60), random features."""
    f0, f1 = features(C, 1, C, 60, 94)
    check(ftk, f0, f1, L, r, coords_for(C + 1, 1, 60, 94))


@pytest.mark.parametrize("B,C,H,W,L,r", [(1, 1, 17, 23, 3, 2), (3, 67, 19, 13, 3, 3), (2, 5, 33, 35, 5, 1), (1, 2, 9, 70, 2, 0)])
def test_odd_sizes_channels_and_batches(ftk, B, C, H, W, L, r):
    """Odd H / W (trailing rows and columns dropped by the pools), C in {1, 67} (odd: the padded last k-step), B > 1 with distinct
    items, a level beyond the fused ones (L 5), r 0."""
    f0, f1 = features(H * W + C, B, C, H, W)
    check(ftk, f0, f1, L, r, coords_for(B * 7 + C, B, H, W))


def test_subnormal_products(ftk):
    """Products of 1e-20-scale features are subnormal (and some round to +-0): the build keeps them, as the fmaf chain does."""
    f0, f1 = features(21, 2, 33, 16, 24, scale=1e-20)
    f0[:, :, :4] *= 1e18  # some rows with normal-range partial sums next to subnormal ones
    check(ftk, f0, f1, 3, 2, coords_for(22, 2, 16, 24))


def test_nan_and_inf_features(ftk):
    f0, f1 = features(31, 1, 16, 16, 20)
    f0[0, 3, 2, 5] = float("nan")
    f1[0, 7, 9, 11] = float("inf")
    f1[0, 8, 9, 12] = float("-inf")
    f0[0, 0, 10, :] = float("inf")
    check(ftk, f0, f1, 3, 2, coords_for(32, 1, 16, 20))


def hostile_case():
    """(fmap0, fmap1, coords) of 1 x 8 x 16 x 24 with NaN, +-inf, huge, 2^31 and edge coordinates over the first 600 of them."""
    f0, f1 = features(41, 1, 8, 16, 24)
    c = coords_for(42, 1, 16, 24)
    flat = c.view(-1)
    specials = torch.tensor([float("nan"), float("inf"), float("-inf"), 1e30, -1e30, 3e9, -3e9, 2.0 ** 31, -0.0, 23.0, 15.0, -1.0])
    flat[: specials.numel() * 50] = specials.repeat(50)
    return f0, f1, c


def test_hostile_coordinates(ftk):
    f0, f1, c = hostile_case()
    check(ftk, f0, f1, 3, 3, c)


def test_level0_volume_larger_than_2_gib(ftk):
    """B 1, 160 x 150 (24 000 pixels): level 0 holds 576 M floats, 2.3 GB; a seeded sample of rows of levels 0 and 1."""
    B, C, H, W = 1, 8, 160, 150
    f0, f1 = features(51, B, C, H, W)
    dev = torch.device("cuda")
    cp = ftk.CorrelationPyramid(f0.to(dev), f1.to(dev), 2, 1)
    assert cp.correlation_pyramid[0].numel() * 4 > 2 ** 31
    rows = np.random.default_rng(52).choice(H * W, 24, replace=False).tolist() + [0, H * W - 1]
    for p in rows:
        want0 = R.row(f0.numpy(), f1.numpy(), 0, p)
        got0 = cp.correlation_pyramid[0][p, 0].cpu().numpy()
        assert R.same(got0, want0), f"row {p}"
        assert R.same(cp.correlation_pyramid[1][p, 0].cpu().numpy(), R.pool(want0[None])[0]), f"row {p}, level 1"
    del cp
    torch.cuda.empty_cache()


def test_non_default_stream(ftk):
    f0, f1 = features(61, 2, 32, 20, 28)
    c = coords_for(62, 2, 20, 28)
    dev = torch.device("cuda")
    s = torch.cuda.Stream()
    a0, a1, ac = f0.to(dev), f1.to(dev), c.to(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        cp = ftk.CorrelationPyramid(a0, a1, 3, 2)
        out = cp.lookup(ac)
    s.synchronize()
    want = R.build(f0.numpy(), f1.numpy(), 3)
    assert R.same(out.cpu().numpy(), R.lookup(want, c.numpy(), 2))


def test_graph_capture_build_and_twelve_lookups(ftk):
    """Build + 12 lookups with the coordinates moved in between (RAFT's refinement loop), captured in one torch.cuda.graph: the replay
    is bit-identical to the eager run."""
    dev = torch.device("cuda")
    f0, f1 = features(71, 2, 64, 24, 32)
    s0, s1 = f0.to(dev), f1.to(dev)
    c0 = coords_for(72, 2, 24, 32).to(dev)
    delta = (torch.randn(2, 2, 24, 32, generator=torch.Generator().manual_seed(73)) * 0.7).to(dev)

    def run(a, b, c):
        cp = ftk.CorrelationPyramid(a, b, 4, 3)
        outs = []
        for _ in range(12):
            outs.append(cp.lookup(c))
            c = c + delta
        return outs

    eager = [o.cpu() for o in run(s0, s1, c0)]
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        run(s0, s1, c0)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        captured = run(s0, s1, c0)
    for o in captured:
        o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for k, (e, o) in enumerate(zip(eager, captured)):
        assert R.same(o.cpu().numpy(), e.numpy()), f"lookup {k}"


def test_fused_lookup_equals_cat_permute(ftk):
    dev = torch.device("cuda")
    f0, f1 = features(81, 2, 16, 12, 20)
    c = coords_for(82, 2, 12, 20).to(dev)
    cp = ftk.CorrelationPyramid(f0.to(dev), f1.to(dev), 3, 2)
    composed = torch.cat(cp(c), dim=-1).permute(0, 3, 1, 2).contiguous()
    assert R.same(cp.lookup(c).cpu().numpy(), composed.cpu().numpy())


def test_against_the_torch_gpu_composition(ftk):
    """The reference's torch arithmetic on the same device (its division by a scalar is a reciprocal multiply there, its BLAS order
    its own): every level within the CPU test's relative bound for level 0; the lookup within the lookup bound plus level 0's plus
    the slope times an ulp of the sample coordinate (its sampler rounds the coordinate differently)."""
    dev = torch.device("cuda")
    f0, f1 = features(91, 1, 128, 60, 94)
    c = coords_for(92, 1, 60, 94).to(dev)
    a0, a1 = f0.to(dev), f1.to(dev)
    cp = ftk.CorrelationPyramid(a0, a1, 3, 3)
    ref = torch_pyramid(a0, a1, 3)
    scale = float(ref[0].abs().max())
    assert float((cp.correlation_pyramid[0] - ref[0]).abs().max()) <= LEVEL0_REL_TOL * scale
    for l in range(1, 3):
        assert float((cp.correlation_pyramid[l] - ref[l]).abs().max()) <= LEVEL0_REL_TOL * scale
    out = cp.lookup(c)
    want = torch_lookup(ref, c, 3)
    # torch CUDA's grid_sample unnormalises as ((g + 1) / 2) * (size - 1), not torch CPU's (g + 1) * ((size - 1) / 2): the sample point
    # moves by up to an ulp of the coordinate, which the bilinear slope (at most 2 max|corr| per pixel) turns into this term
    coord_ulp = 2.0 ** -23 * max(60, 94)
    assert float((out - want).abs().max()) <= (LOOKUP_TOL + LEVEL0_REL_TOL + 2 * coord_ulp) * scale


def test_inference_only_and_loud_errors(ftk):
    dev = torch.device("cuda")
    f = torch.randn(1, 4, 8, 8, device=dev)
    with pytest.raises(ValueError, match="same size"):
        ftk.CorrelationPyramid(f, torch.randn(1, 4, 8, 9, device=dev), 2, 1)
    with pytest.raises(ValueError, match="float32"):
        ftk.CorrelationPyramid(f.double(), f.double(), 2, 1)
    with pytest.raises(ValueError, match="avg_pool2d"):
        ftk.CorrelationPyramid(f, f, 5, 1)  # 8 -> 4 -> 2 -> 1 -> 0
    g = f.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        ftk.CorrelationPyramid(g, f, 2, 1)
    with torch.no_grad():
        cp = ftk.CorrelationPyramid(g, f, 2, 1)
    with pytest.raises(ValueError, match="pixel_locations"):
        cp.lookup(torch.zeros(1, 3, 8, 8, device=dev))
