"""RAFT's correlation pyramid without a device: the scalar restatement (tests/raft_corr_ref.c) pinned against the
reference's own arithmetic (a torch CPU composition that follows correlation_volumes.py step by step, and, where a checkout of the
reference is present, its CorrelationPyramid class itself), known answers, the host-only layout entry, and the loud failures."""
import importlib.util
import os

import numpy as np
import pytest

from tests import raft_corr_ref as R

torch = pytest.importorskip("torch")

REFERENCE_DIR = os.environ.get("FEATURE_TRACKER_REFERENCE_DIR", "/root/reference")
REFERENCE_CORR = os.path.join(REFERENCE_DIR, "src", "nn_optical_flow_tracker", "raft", "correlation_volumes.py")

# The sampler is pinned to torch CPU's grid_sample within this bound, scaled by max |corr|.  On torch 2.10 CPU the
# restatement's sampler was bit-identical; the bound leaves room for a torch build whose vector path contracts differently.
LOOKUP_TOL = 1e-6
LEVEL0_REL_TOL = 2e-6  # random features: torch's BLAS sums the channels in its own order


def torch_pyramid(f0, f1, levels):
    """correlation_volumes.py:20-46 on CPU: matmul, / channels ** 0.5, avg_pool2d."""
    B, C, H, W = f0.shape
    corr = torch.matmul(f0.view(B, C, H * W).transpose(1, 2), f1.view(B, C, H * W))
    corr = corr.view(B, H, W, 1, H, W) / (C ** 0.5)
    out = [corr.view(B * H * W, 1, H, W)]
    for _ in range(levels - 1):
        out.append(torch.nn.functional.avg_pool2d(out[-1], kernel_size=2, stride=2))
    return out


def torch_lookup(pyramid, coords, r):
    """correlation_volumes.py:3-17 and 48-77, then model.py:88: [B, L*K, H, W]."""
    loc = coords.permute(0, 2, 3, 1)
    B, H, W, _ = loc.shape
    outs = []
    for i, corr in enumerate(pyramid):
        d = torch.linspace(-r, r, 2 * r + 1)
        dy, dx = torch.meshgrid(d, d, indexing="ij")
        neighbors = torch.stack([dx, dy], dim=-1).reshape(1, 2 * r + 1, 2 * r + 1, 2).to(corr.device)
        pts = (loc / 2 ** i).reshape(B * H * W, 1, 1, 2) + neighbors
        h, w = corr.shape[-2:]
        x, y = pts.split([1, 1], dim=-1)
        grid = torch.cat([2 * x / (w - 1) - 1, 2 * y / (h - 1) - 1], dim=-1)
        s = torch.nn.functional.grid_sample(corr, grid, align_corners=True)
        outs.append(s.view(B, H, W, (2 * r + 1) ** 2))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def levels_np(pyr):
    return [p[:, 0].numpy() for p in pyr]


def random_coords(g, B, H, W, spread=1.4, shift=-3.0):
    scale = torch.tensor([W, H], dtype=torch.float32).view(1, 2, 1, 1)
    return (torch.rand(B, 2, H, W, generator=g) * scale * spread + shift).float()


@pytest.mark.parametrize("C", [1, 3, 67, 128, 256])
def test_level0_small_integer_features_bit_identical(C):
    """Every dot product is exact, so only the division is compared: torch's `/ channels ** 0.5` is the true division by
    (float)sqrt((double)C) (a reciprocal multiply differs for C = 3, 67, 128)."""
    g = torch.Generator().manual_seed(C)
    f0 = torch.randint(-4, 5, (2, C, 5, 7), generator=g).float()
    f1 = torch.randint(-4, 5, (2, C, 5, 7), generator=g).float()
    mine = R.build(f0.numpy(), f1.numpy(), 1)
    assert R.same(mine[0], torch_pyramid(f0, f1, 1)[0][:, 0].numpy())


def test_level0_random_features_within_bound():
    g = torch.Generator().manual_seed(7)
    f0, f1 = torch.randn(2, 128, 12, 17, generator=g), torch.randn(2, 128, 12, 17, generator=g)
    mine = R.build(f0.numpy(), f1.numpy(), 1)[0]
    ref = torch_pyramid(f0, f1, 1)[0][:, 0].numpy()
    assert np.abs(mine - ref).max() <= LEVEL0_REL_TOL * np.abs(ref).max()


def test_pooled_levels_bit_identical_from_the_same_level0():
    g = torch.Generator().manual_seed(3)
    f0, f1 = torch.randn(2, 32, 23, 21, generator=g), torch.randn(2, 32, 23, 21, generator=g)
    pyr = torch_pyramid(f0, f1, 4)
    for l in range(1, 4):
        assert R.same(R.pool(pyr[l - 1][:, 0].numpy()), pyr[l][:, 0].numpy()), f"level {l}"


@pytest.mark.parametrize("shape", [(5, 128, 8, 8, 3, 3), (2, 67, 13, 11, 3, 2), (1, 32, 20, 31, 4, 4)])
def test_lookup_against_torch_grid_sample(shape):
    B, C, H, W, L, r = shape
    g = torch.Generator().manual_seed(H * W)
    f0, f1 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    pyr = torch_pyramid(f0, f1, L)
    coords = random_coords(g, B, H, W)
    ref = torch_lookup(pyr, coords, r).numpy()
    mine = R.lookup(levels_np(pyr), coords.numpy(), r)
    scale = max(float(np.abs(p.numpy()).max()) for p in pyr)
    assert mine.shape == ref.shape
    assert np.abs(mine - ref).max() <= LOOKUP_TOL * scale


@pytest.mark.skipif(not os.path.exists(REFERENCE_CORR), reason="the reference checkout is not present")
def test_against_the_reference_class():
    """The reference's own CorrelationPyramid (its __main__ shape: B 5, C 128, 8 x 8, 3 levels, r 3) on CPU."""
    spec = importlib.util.spec_from_file_location("reference_correlation_volumes", REFERENCE_CORR)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = torch.Generator().manual_seed(5)
    f0, f1 = torch.randn(5, 128, 8, 8, generator=g), torch.randn(5, 128, 8, 8, generator=g)
    ref = mod.CorrelationPyramid(f0, f1, num_levels=3, radius=3)
    mine = R.build(f0.numpy(), f1.numpy(), 3)
    r0 = ref.correlation_pyramid[0][:, 0].numpy()
    assert np.abs(mine[0] - r0).max() <= LEVEL0_REL_TOL * np.abs(r0).max()
    for l in range(1, 3):
        assert R.same(R.pool(ref.correlation_pyramid[l - 1][:, 0].numpy()), ref.correlation_pyramid[l][:, 0].numpy())
    coords = random_coords(g, 5, 8, 8)
    out = torch.cat(ref(coords), dim=-1).permute(0, 3, 1, 2).contiguous().numpy()
    mine_out = R.lookup(levels_np(ref.correlation_pyramid), coords.numpy(), 3)
    assert np.abs(mine_out - out).max() <= LOOKUP_TOL * max(float(np.abs(p.numpy()).max()) for p in ref.correlation_pyramid)


def test_linear_volume_returns_the_sample_coordinates():
    """A level whose slab is v(x, y) = x + 100 y: the sample of channel i * (2r+1) + j is (x / 2^l + j - r) + 100 (y / 2^l + i - r),
    which checks the window order (i with y, j with x) and the / 2^l scaling."""
    H, W, r = 32, 48, 1
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    levels = []
    for l, (h, w) in enumerate(R.layout(H, W, 3)):
        y, x = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
        levels.append(np.broadcast_to(x + 100 * y, (H * W, h, w)).copy())
    coords = np.stack([xx * 0 + 18.5, yy * 0 + 12.25])[None].astype(np.float32)  # the window stays inside every level
    out = R.lookup(levels, coords, r)
    side = 2 * r + 1
    for l in range(3):
        for i in range(side):
            for j in range(side):
                want = (18.5 / 2 ** l + j - r) + 100 * (12.25 / 2 ** l + i - r)
                got = out[0, l * side * side + i * side + j]
                assert np.allclose(got, want, rtol=0, atol=1e-3), (l, i, j, float(got[0, 0]), want)


def test_width_one_level_is_nan():
    """W_l == 1 divides by W_l - 1 == 0 exactly as the reference does: every sample of that level is NaN."""
    g = torch.Generator().manual_seed(11)
    f0, f1 = torch.randn(1, 4, 8, 3, generator=g), torch.randn(1, 4, 8, 3, generator=g)
    pyr = torch_pyramid(f0, f1, 2)
    assert pyr[1].shape[-1] == 1
    coords = random_coords(g, 1, 8, 3)
    mine = R.lookup(levels_np(pyr), coords.numpy(), 1)
    assert np.isnan(mine[:, 9:]).all() and not np.isnan(mine[:, :9]).any()
    assert R.same(mine, torch_lookup(pyr, coords, 1).numpy())


def test_hostile_coordinates():
    """NaN / inf coordinates give NaN (through the weights), huge finite ones 0 (every corner outside); none reads memory."""
    slab = np.arange(35, dtype=np.float32).reshape(5, 7)
    for x, y, want in [(np.nan, 2.0, "nan"), (2.0, np.inf, "nan"), (-np.inf, 2.0, "nan"), (1e30, 2.0, 0.0), (2.0, -1e30, 0.0), (-1e30, 1e30, 0.0)]:
        v = R.sample(slab, 0, x, y, 0, 0)
        assert (np.isnan(v) if want == "nan" else v == want), (x, y, v)
    # just outside the last column: only the west corners are inside
    v = R.sample(slab, 0, 6.5, 1.0, 0, 0)
    assert v == np.float32(0.5) * slab[1, 6]


def test_empty_level_is_refused():
    from feature_tracker_amd import _native
    with pytest.raises(_native.FtkError, match="avg_pool2d"):
        _native.corr_pyramid_layout(1, 6, 9, 4)  # 6 -> 3 -> 1 -> 0
    with pytest.raises(_native.FtkError):
        _native.corr_pyramid_layout(1, 8, 8, 0)
    with pytest.raises(_native.FtkError):
        _native.corr_pyramid_layout(1, 8, 8, _native.FTK_CORR_MAX_LEVELS + 1)


def test_layout_sizes_and_offsets():
    from feature_tracker_amd import _native
    B, H, W, L = 2, 60, 94, 4
    elements, offsets, dims = _native.corr_pyramid_layout(B, H, W, L)
    assert dims == [(60, 94), (30, 47), (15, 23), (7, 11)]
    n = B * H * W
    sizes = [n * h * w for h, w in dims]
    assert offsets == [sum(sizes[:l]) for l in range(L)]
    assert elements == sum(sizes) == n * sum(h * w for h, w in dims)
    # the C ABI's byte count, 4 * B * H * W * sum H_l W_l, past 2^31 bytes
    big, _, _ = _native.corr_pyramid_layout(1, 160, 150, 1)
    assert 4 * big > 2 ** 31


def test_class_fails_loudly_without_a_device():
    import feature_tracker_amd as F
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    f = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.CorrelationPyramid(f, f, 2, 1)
