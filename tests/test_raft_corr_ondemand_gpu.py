"""OnDemandCorrelation on the device against the scalar restatement (tests/raft_corr_ondemand_ref.c): both output forms are bit-identical
(any NaN equals any NaN) at odd sizes, channel counts below and off the vector width, several batch items, five levels,
radius 0, a radius above the lattice's (every corner evaluated directly), a level of width 2, windows outside every level, subnormal,
NaN / inf and hostile inputs, and the coordinates the CPU search found the lattice trap at; level 0 equals CorrelationPyramid's bit for
bit; and construction allocates the workspace the formula gives, a small fraction of the volume."""
import numpy as np
import pytest

from tests import raft_corr_ondemand_ref as O
from tests.test_raft_corr_ondemand_cpu import TRAP_RADIUS, lattice_trap_coordinates

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def features(seed, B, C, H, W, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, C, H, W, generator=g) * scale).float(), (torch.randn(B, C, H, W, generator=g) * scale).float()


def coords_for(seed, B, H, W, spread=1.4, shift=-3.0):
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([W, H], dtype=torch.float32).view(1, 2, 1, 1)
    return (torch.rand(B, 2, H, W, generator=g) * scale * spread + shift).float()


def where_differs(got, want):
    return np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5].tolist()


def check(ftk, f0, f1, L, r, coords):
    """Both lookup forms of the device object against the restatement, bit for bit; returns the object and the fused result."""
    dev = torch.device("cuda")
    od = ftk.OnDemandCorrelation(f0.to(dev), f1.to(dev), L, r)
    assert (od.num_levels, od.radius) == (L, r) and not hasattr(od, "correlation_pyramid")
    want = O.lookup(f0.numpy(), f1.numpy(), L, coords.numpy(), r)
    fused = od.lookup(coords.to(dev))
    K = (2 * r + 1) ** 2
    assert fused.is_contiguous() and fused.dtype == torch.float32 and tuple(fused.shape) == (f0.shape[0], L * K, f0.shape[2], f0.shape[3])
    got = fused.cpu().numpy()
    assert O.same(got, want), f"lookup differs at {where_differs(got, want)}"
    per_level = od(coords.to(dev))
    assert len(per_level) == L
    for l, t in enumerate(per_level):
        assert t.is_contiguous() and tuple(t.shape) == (f0.shape[0], f0.shape[2], f0.shape[3], K)
        assert O.same(t.cpu().numpy(), np.moveaxis(want[:, l * K:(l + 1) * K], 1, -1)), f"per-level form, level {l}"
    return od, got


def test_reference_main_shape(ftk):
    """correlation_volumes.py's __main__: B 5, C 128, 8 x 8, 3 levels, r 3."""
    f0, f1 = features(1, 5, 128, 8, 8)
    check(ftk, f0, f1, 3, 3, coords_for(2, 5, 8, 8))


@pytest.mark.parametrize("B,C,H,W,L,r", [(1, 1, 17, 23, 3, 2), (3, 67, 19, 13, 3, 3), (2, 5, 33, 35, 5, 1), (1, 2, 9, 70, 2, 0)])
def test_odd_sizes_channels_and_batches(ftk, B, C, H, W, L, r):
    """Odd H / W (the pools drop the trailing row and column), C below and off the vector width, B > 1 with distinct items, five levels,
    r 0."""
    f0, f1 = features(H * W + C, B, C, H, W)
    check(ftk, f0, f1, L, r, coords_for(B * 7 + C, B, H, W))


def test_production_channel_count(ftk):
    """C 256 at a small map, r 4: two passes over the 100 lattice points, 16-byte loads."""
    f0, f1 = features(5, 1, 256, 12, 20)
    check(ftk, f0, f1, 3, 4, coords_for(6, 1, 12, 20))


def test_radius_above_the_lattice(ftk):
    """r 8: 2r + 2 = 18 is wider than the lattice a wave keeps, so every corner of every sample is evaluated directly."""
    f0, f1 = features(7, 1, 3, 20, 24)
    check(ftk, f0, f1, 2, 8, coords_for(8, 1, 20, 24))


def test_level_of_width_and_height_two(ftk):
    """H 4, W 9, L 2: level 1 is 2 x 4, (h - 1) / 2 = 0.5; and H 9, W 4 for a width of 2."""
    for H, W in ((4, 9), (9, 4)):
        f0, f1 = features(9 + H, 1, 8, H, W)
        check(ftk, f0, f1, 2, 2, coords_for(10, 1, H, W))


def test_windows_outside_every_level(ftk):
    f0, f1 = features(11, 2, 8, 10, 14)
    c = coords_for(12, 2, 10, 14)
    c[0] += 100.0   # far to the south-east of every level
    c[1] = -50.0 - c[1]
    _, got = check(ftk, f0, f1, 3, 2, c)
    assert not got.any()  # all exactly zero


def test_subnormal_products(ftk):
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


def test_hostile_coordinates(ftk):
    f0, f1 = features(41, 1, 8, 16, 24)
    c = coords_for(42, 1, 16, 24)
    flat = c.view(-1)
    specials = torch.tensor([float("nan"), float("inf"), float("-inf"), 1e30, -1e30, 3e9, -3e9, 2.0 ** 31, -0.0, 23.0, 15.0, -1.0])
    flat[: specials.numel() * 50] = specials.repeat(50)
    check(ftk, f0, f1, 3, 3, c)


def test_lattice_trap_coordinates(ftk):
    """The coordinates at which the CPU search found floor(ix) at offset dj + 1 != floor(ix) at dj plus one, as x and as y of square maps of
    those widths, and integer coordinates (RAFT's first iteration), where half the traps are."""
    traps = lattice_trap_coordinates()
    if not traps:
        pytest.skip("the CPU search found no trap in its range: nothing to reuse")
    for w, xs in traps.items():
        f0, f1 = features(50 + w, 1, 8, w, w)
        c = coords_for(51 + w, 1, w, w)
        vals = torch.tensor(xs, dtype=torch.float32)
        n = w * w
        c[0, 0].view(-1)[:] = vals.repeat(n // len(xs) + 1)[:n]
        c[0, 1].view(-1)[: n // 2] = vals.repeat(n // len(xs) + 1)[: n // 2]
        check(ftk, f0, f1, 1, TRAP_RADIUS, c)
    ys, xs = torch.meshgrid(torch.arange(23.0), torch.arange(29.0), indexing="ij")
    f0, f1 = features(60, 1, 8, 23, 29)
    check(ftk, f0, f1, 3, TRAP_RADIUS, torch.stack([xs, ys])[None].contiguous())


def test_level_0_equals_the_correlation_pyramid(ftk):
    dev = torch.device("cuda")
    f0, f1 = features(71, 2, 64, 24, 32)
    c = coords_for(72, 2, 24, 32).to(dev)
    L, r = 3, 3
    K = (2 * r + 1) ** 2
    od = ftk.OnDemandCorrelation(f0.to(dev), f1.to(dev), L, r).lookup(c).cpu().numpy()
    ap = ftk.CorrelationPyramid(f0.to(dev), f1.to(dev), L, r).lookup(c).cpu().numpy()
    assert O.same(od[:, :K], ap[:, :K])
    assert float(np.abs(od[:, K:] - ap[:, K:]).max()) < 1e-4 * float(np.abs(ap).max())  # the same quantity, other roundings


def test_construction_allocates_the_workspace_and_no_volume(ftk):
    from feature_tracker_amd import _native as N
    dev = torch.device("cuda")
    B, C, H, W, L = 1, 64, 48, 64, 3
    f0, f1 = (t.to(dev) for t in features(81, B, C, H, W))
    ftk.OnDemandCorrelation(f0[:, :4, :8, :8].contiguous(), f1[:, :4, :8, :8].contiguous(), 1, 1)  # the library context exists from here on
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    od = ftk.OnDemandCorrelation(f0, f1, L, 4)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    dims = [(H >> l, W >> l) for l in range(L)]
    assert od.workspace_bytes == 4 * B * C * (H * W + sum(h * w for h, w in dims)) == 4 * N.corr_ondemand_layout(B, C, H, W, L)[0]
    allocator_block = 512  # torch's caching allocator rounds a request up to a multiple of this
    assert 0 < grown <= od.workspace_bytes + allocator_block, (grown, od.workspace_bytes)
    volume_bytes = 4 * N.corr_pyramid_layout(B, H, W, L)[0]
    assert volume_bytes == 4 * B * H * W * sum(h * w for h, w in dims)
    assert grown < volume_bytes / 10, (grown, volume_bytes)  # by the two formulas about C (1 + HW / sum) / HW of it


def test_non_default_stream_and_loud_errors(ftk):
    dev = torch.device("cuda")
    f0, f1 = features(91, 2, 32, 20, 28)
    c = coords_for(92, 2, 20, 28)
    s = torch.cuda.Stream()
    a0, a1, ac = f0.to(dev), f1.to(dev), c.to(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out = ftk.OnDemandCorrelation(a0, a1, 3, 2).lookup(ac)
    s.synchronize()
    assert O.same(out.cpu().numpy(), O.lookup(f0.numpy(), f1.numpy(), 3, c.numpy(), 2))
    f = torch.randn(1, 4, 8, 8, device=dev)
    with pytest.raises(ValueError, match="same size"):
        ftk.OnDemandCorrelation(f, torch.randn(1, 4, 8, 9, device=dev), 2, 1)
    with pytest.raises(ValueError, match="float32"):
        ftk.OnDemandCorrelation(f.double(), f.double(), 2, 1)
    with pytest.raises(ValueError, match="avg_pool2d"):
        ftk.OnDemandCorrelation(f, f, 5, 1)  # 8 -> 4 -> 2 -> 1 -> 0
    with pytest.raises(ValueError, match="radius 65"):
        ftk.OnDemandCorrelation(f, f, 2, 65)
    g = f.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        ftk.OnDemandCorrelation(g, f, 2, 1)
    with torch.no_grad():
        od = ftk.OnDemandCorrelation(g, f, 2, 1)
    with pytest.raises(ValueError, match="pixel_locations"):
        od.lookup(torch.zeros(1, 3, 8, 8, device=dev))
