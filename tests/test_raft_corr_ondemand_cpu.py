"""RAFT's on-demand correlation without a device: the scalar restatement (tests/raft_corr_ondemand_ref.c) held to the
reference's own composition in float64 (matmul, divide, avg_pool2d of the VOLUME, grid_sample: tests/test_raft_corr_cpu.py's) within twice
the error the all-pairs restatement has against it on the same inputs, three mutants of that composition that the same check must reject,
level 0 bit-identical to the all-pairs restatement, the search for the lattice trap (windows whose floors do not step by one), the host-only
layout entry, the loud failures of the Python entries before any device is touched, and the launch plan through its command-line tool."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import raft_corr_ondemand_ref as O
from tests import raft_corr_ref as R

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402
from tests.test_raft_corr_cpu import random_coords, torch_pyramid  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_CLI = os.path.join(ROOT, "feature_tracker_amd", "host", "build", "corr_ondemand_plan_cli")

# The restatement's extra roundings over the all-pairs one are one per channel per pooled level (the pool of fmap1 before the chain, instead
# of the pool of the finished correlation values), so it is allowed twice the all-pairs restatement's own error against float64, per level.
ALLOWED_FACTOR = 2.0
FLOAT64_CASE = (2, 128, 12, 20, 3, 3)  # B, C, H, W, levels, radius


def lookup64(pyramid, coords, r, swap_offsets=False):
    """tests/test_raft_corr_cpu.py::torch_lookup in the pyramid's dtype; ``swap_offsets`` is the mutant that adds dy to x and dx to y."""
    loc = coords.permute(0, 2, 3, 1)
    B, H, W, _ = loc.shape
    outs = []
    for i, corr in enumerate(pyramid):
        d = torch.linspace(-r, r, 2 * r + 1, dtype=corr.dtype)
        dy, dx = torch.meshgrid(d, d, indexing="ij")
        neighbors = torch.stack([dy, dx] if swap_offsets else [dx, dy], dim=-1).reshape(1, 2 * r + 1, 2 * r + 1, 2)
        pts = (loc / 2 ** i).reshape(B * H * W, 1, 1, 2) + neighbors
        h, w = corr.shape[-2:]
        x, y = pts.split([1, 1], dim=-1)
        grid = torch.cat([2 * x / (w - 1) - 1, 2 * y / (h - 1) - 1], dim=-1)
        s = torch.nn.functional.grid_sample(corr, grid, align_corners=True)
        outs.append(s.view(B, H, W, (2 * r + 1) ** 2))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def composition64(f0, f1, levels, coords, r, mutant=None):
    """The reference's composition in float64; ``mutant`` in (None, "shifted pool", "divisor C", "offsets swapped")."""
    f0, f1, coords = f0.double(), f1.double(), coords.double()
    if mutant == "shifted pool":
        B, C, H, W = f0.shape
        corr = torch.matmul(f0.view(B, C, H * W).transpose(1, 2), f1.view(B, C, H * W)).view(B * H * W, 1, H, W) / (C ** 0.5)
        pyramid = [corr]
        for _ in range(levels - 1):  # the 2 x 2 block one pixel down and to the right
            pyramid.append(torch.nn.functional.avg_pool2d(torch.roll(pyramid[-1], shifts=(-1, -1), dims=(-2, -1)), kernel_size=2, stride=2))
    else:
        pyramid = torch_pyramid(f0, f1, levels)
        if mutant == "divisor C":
            pyramid = [p / (f0.shape[1] ** 0.5) for p in pyramid]
    return lookup64(pyramid, coords, r, swap_offsets=mutant == "offsets swapped").numpy()


@functools.lru_cache(maxsize=None)
def float64_case():
    """Inputs, the float64 yardstick and both restatements' outputs at FLOAT64_CASE: computed once and shared; nobody writes to them."""
    B, C, H, W, L, r = FLOAT64_CASE
    g = torch.Generator().manual_seed(2024)
    f0, f1 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    coords = random_coords(g, B, H, W)
    ref64 = composition64(f0, f1, L, coords, r)
    all_pairs = R.lookup(R.build(f0.numpy(), f1.numpy(), L), coords.numpy(), r)
    on_demand = O.lookup(f0.numpy(), f1.numpy(), L, coords.numpy(), r)
    return f0, f1, coords, ref64, all_pairs, on_demand


def per_level_error(out, ref64, levels):
    K = out.shape[1] // levels
    return [float(np.abs(out[:, l * K:(l + 1) * K].astype(np.float64) - ref64[:, l * K:(l + 1) * K]).max()) for l in range(levels)]


def within_the_bound(candidate, ref64, all_pairs_error, levels):
    """The check of this file: per level, the candidate's largest error against float64 is at most twice the all-pairs restatement's."""
    return [e <= ALLOWED_FACTOR * a for e, a in zip(per_level_error(candidate, ref64, levels), all_pairs_error)]


def test_restatement_against_float64_within_twice_the_all_pairs_error():
    _, _, _, ref64, all_pairs, on_demand = float64_case()
    L = FLOAT64_CASE[4]
    base, mine = per_level_error(all_pairs, ref64, L), per_level_error(on_demand, ref64, L)
    for l in range(L):
        print(f"level {l}: all-pairs restatement vs float64 {base[l]:.3g}, on-demand restatement vs float64 {mine[l]:.3g} "
              f"({mine[l] / base[l]:.2f} x, allowed {ALLOWED_FACTOR} x)")
    assert all(b > 0 for b in base)  # float32 arithmetic has an error to compare with
    assert all(within_the_bound(on_demand, ref64, base, L)), (base, mine)


def test_level_0_is_bit_identical_to_the_all_pairs_restatement():
    _, _, _, _, all_pairs, on_demand = float64_case()
    K = (2 * FLOAT64_CASE[5] + 1) ** 2
    assert R.same(on_demand[:, :K], all_pairs[:, :K])
    assert not R.same(on_demand[:, K:], all_pairs[:, K:])  # the pooled levels round differently: the two are not one computation


@pytest.mark.parametrize("mutant", ["shifted pool", "divisor C", "offsets swapped"])
def test_mutants_of_the_composition_fail_the_bound(mutant):
    """The check can fail: each mutant, even evaluated in float64, is further from the yardstick than the bound allows."""
    f0, f1, coords, ref64, all_pairs, _ = float64_case()
    B, C, H, W, L, r = FLOAT64_CASE
    base = per_level_error(all_pairs, ref64, L)
    ok = within_the_bound(composition64(f0, f1, L, coords, r, mutant).astype(np.float32), ref64, base, L)
    print(f"mutant {mutant}: within the bound per level {ok}")
    assert not all(ok)
    if mutant == "shifted pool":
        assert ok[0] and not any(ok[1:])  # level 0 has no pool
    else:
        assert not any(ok)


def test_pool_and_row_known_answers():
    fmap = np.arange(2 * 3 * 5 * 7, dtype=np.float32).reshape(2, 3, 5, 7)
    pooled = O.pool(fmap)
    assert pooled.shape == (2, 3, 2, 3)  # the trailing row and column are dropped
    assert pooled[1, 2, 1, 2] == (((fmap[1, 2, 2, 4] + fmap[1, 2, 2, 5]) + fmap[1, 2, 3, 4]) + fmap[1, 2, 3, 5]) / np.float32(4)
    g = np.random.default_rng(3)
    f0, f1 = g.standard_normal((2, 5, 4, 6)).astype(np.float32), g.standard_normal((2, 5, 4, 6)).astype(np.float32)
    assert R.same(O.row(f0, f1, 1, 7), R.row(f0, f1, 1, 7))  # level 0: rcr_row itself
    # a position outside the level is 0, a NaN coordinate NaN, as in the all-pairs sampler
    slab = np.arange(35, dtype=np.float32).reshape(5, 7)
    assert O.sample(slab, 0, 6.5, 1.0, 0, 0) == np.float32(0.5) * slab[1, 6]
    assert O.sample(slab, 0, 1e30, 2.0, 0, 0) == 0 and np.isnan(O.sample(slab, 0, np.nan, 2.0, 0, 0))
    for args in ((0, 3.25, 1.5, 1, -1), (1, 5.75, 2.5, 0, 1), (2, -1.0, 30.0, -2, 2)):
        assert R.same(np.float32([O.sample(slab, *args)]), np.float32([R.sample(slab, *args)]))


# ---- the lattice trap ---------------------------------------------------------------------------------------------------------------

TRAP_RADIUS = 4


@functools.lru_cache(maxsize=None)
def lattice_trap_cases():
    """Every (w, x, dj) found, level 0, with floor(ix) at offset dj + 1 != floor(ix) at dj plus one, by the restatement's own sampler, over
    level widths 2 .. 130 and coordinates at, one ulp below and one ulp above every integer of -2 .. w + 1 and w - 1 +- a few ulps."""
    found = []
    for w in range(2, 131):
        ints = np.arange(-2, w + 2, dtype=np.float32)
        near_last = np.float32(w - 1) + np.float32(w - 1) * np.float32(2.0 ** -23) * np.arange(-4, 5, dtype=np.float32)
        xs = np.unique(np.concatenate([ints, np.nextafter(ints, np.float32(-np.inf)), np.nextafter(ints, np.float32(np.inf)), near_last.astype(np.float32)]))
        floors = {dj: O.floor_ix(w, 0, xs, dj) for dj in range(-TRAP_RADIUS, TRAP_RADIUS + 1)}
        for dj in range(-TRAP_RADIUS, TRAP_RADIUS):
            bad = np.isfinite(floors[dj]) & (floors[dj + 1] != floors[dj] + 1)
            found += [(w, float(x), dj) for x in xs[bad]]
    return tuple(found)


def lattice_trap_coordinates(limit=3, narrowest=12, widest=48):
    """For the GPU test: {w: coordinates} of up to ``limit`` level widths in ``narrowest`` .. ``widest`` (the first, the middle and the last
    one the search found a trap at): maps wide enough for a window to lie inside, small enough for a quick test."""
    by_width = {}
    for w, x, _ in lattice_trap_cases():
        if narrowest <= w <= widest:
            by_width.setdefault(w, []).append(x)
    widths = sorted(by_width)
    picked = sorted({widths[0], widths[len(widths) // 2], widths[-1]})[:limit] if widths else []
    return {w: sorted(set(by_width[w])) for w in picked}


def test_lattice_trap_search():
    cases = lattice_trap_cases()
    print(f"lattice trap: {len(cases)} (w, x, dj) with floor(ix(dj + 1)) != floor(ix(dj)) + 1; widths {sorted({c[0] for c in cases})[:12]} ...; "
          f"first {cases[:3]}")
    if not cases:
        assert lattice_trap_coordinates() == {}  # nothing for the GPU test to reuse
        return
    # what was found is real: re-evaluated one by one through the sampler's floors
    for w, x, dj in cases[:50]:
        a, b = O.floor_ix(w, 0, [x], dj)[0], O.floor_ix(w, 0, [x], dj + 1)[0]
        assert b != a + 1, (w, x, dj, a, b)
    assert lattice_trap_coordinates(), "traps were found, but at no width the GPU test can afford"


# ---- the layout ---------------------------------------------------------------------------------------------------------------------


def test_layout_sizes_and_offsets_for_odd_sizes():
    from feature_tracker_amd import _native as N
    for B, C, H, W, L in ((2, 5, 33, 35, 5), (1, 67, 19, 13, 3), (3, 1, 9, 70, 2), (1, 256, 55, 128, 4)):
        elements, offsets, dims = N.corr_ondemand_layout(B, C, H, W, L)
        assert dims == R.layout(H, W, L) == N.corr_pyramid_layout(B, H, W, L)[2]
        sizes = [B * C * h * w for h, w in dims]
        assert offsets == [B * C * H * W + sum(sizes[:l]) for l in range(L)]  # fmap0 transposed comes first
        assert elements == B * C * (H * W + sum(h * w for h, w in dims))
    assert N.corr_ondemand_layout(2, 5, 33, 35, 5)[2] == [(33, 35), (16, 17), (8, 8), (4, 4), (2, 2)]


def test_layout_errors():
    from feature_tracker_amd import _native as N
    with pytest.raises(N.FtkError, match="avg_pool2d"):
        N.corr_ondemand_layout(1, 4, 6, 9, 4)  # 6 -> 3 -> 1 -> 0
    with pytest.raises(N.FtkError, match="level 3 .* use at most 3 levels"):
        N.corr_ondemand_layout(1, 4, 6, 9, 4)
    for levels in (0, -1, N.FTK_CORR_MAX_LEVELS + 1):
        with pytest.raises(N.FtkError, match=r"levels \(1 \.\. 16\)"):
            N.corr_ondemand_layout(1, 4, 8, 8, levels)
    for B, C, H, W in ((0, 4, 8, 8), (1, 4, 0, 8), (1, 4, 8, -3)):
        with pytest.raises(N.FtkError, match="must be positive"):
            N.corr_ondemand_layout(B, C, H, W, 1)
    with pytest.raises(N.FtkError, match="0 channels"):
        N.corr_ondemand_layout(1, 0, 8, 8, 1)
    with pytest.raises(N.FtkError, match="byte count"):
        N.corr_ondemand_layout(2 ** 15, 2 ** 30, 2 ** 15, 2 ** 15, 1)
    # 1080p features, B 1, C 256: 77 MB where the volume is 5.6 GB
    elements, _, _ = N.corr_ondemand_layout(1, 256, 135, 240, 4)
    volume, _, _ = N.corr_pyramid_layout(1, 135, 240, 4)
    assert 4 * elements < 80e6 and 4 * volume > 5e9


# ---- loud failures, before any device is touched --------------------------------------------------------------------------------------


def test_class_refuses_bad_arguments_without_a_device():
    import feature_tracker_amd as F
    f = torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError, match="fmap0 must be a 4-D float32 CUDA tensor"):
        F.OnDemandCorrelation(f, f, 2, 1)  # CPU tensors
    with pytest.raises(ValueError, match="fmap1 must be a 4-D float32 CUDA tensor"):
        F.OnDemandCorrelation(f, f.double(), 2, 1)
    with pytest.raises(ValueError, match="fmap0 must be a 4-D float32 CUDA tensor"):
        F.OnDemandCorrelation(f[0], f, 2, 1)
    with pytest.raises(ValueError, match="fmap0 must be"):
        F.OnDemandCorrelation(f.numpy(), f, 2, 1)
    with pytest.raises(ValueError, match="must have the same size and device"):
        F.OnDemandCorrelation(f, torch.zeros(1, 4, 8, 9), 2, 1)
    assert not hasattr(F.OnDemandCorrelation, "correlation_pyramid")
    assert isinstance(F.OnDemandCorrelation.workspace_bytes, property)
    assert "OnDemandCorrelation" in F.__all__


def test_raft_refuses_a_bad_mode_and_bad_images_without_a_device():
    import feature_tracker_amd as F
    from tests.test_raft_encoder_cpu import RAFT_CASES, make_image, make_raft_state
    c = RAFT_CASES[0]
    state = make_raft_state(c, 1)
    for bad in ("on-demand", "alternate", "", None, 1):
        with pytest.raises(ValueError, match="correlation .* is not one of 'all_pairs', 'on_demand'"):
            F.Raft.from_state_dict(state, c[3], c[4], correlation=bad)
    default = F.Raft.from_state_dict(state, c[3], c[4])
    assert default.correlation == "all_pairs"
    with pytest.raises(ValueError, match="is not one of"):
        F.Raft(default.feature_encoder, default.context_encoder, default.update_block, c[3], c[4], correlation="volume")
    model = F.Raft.from_state_dict(state, c[3], c[4], max_iterations=2, correlation="on_demand")
    assert model.correlation == "on_demand"
    ref, cur = make_image(1, 1, 16, 24, 1), make_image(1, 1, 16, 24, 2)
    with pytest.raises(ValueError, match="ref_image must be"):
        model(ref.double(), cur)
    with pytest.raises(ValueError, match="The size of the reference and current images should be the same"):
        model(ref, cur[:, :, :15])
    with pytest.raises(ValueError, match="no CPU fallback"):
        model(ref, cur)  # CPU tensors


def test_on_demand_raft_checks_the_levels_without_sizing_a_volume(monkeypatch):
    """With "on_demand" the level rules are asked of the workspace layout; the volume's layout entry is never called."""
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from tests.test_raft_encoder_cpu import RAFT_CASES, make_image, make_raft_state
    c = RAFT_CASES[0]
    state = make_raft_state((c[0], c[1], c[2], 3, 0) + tuple(c[5:]), 1)  # 3 levels of radius 0: 3 correlation channels
    model = F.Raft.from_state_dict(state, 3, 0, correlation="on_demand")

    def never(*args):
        raise AssertionError("corr_pyramid_layout was called")

    from feature_tracker_amd import raft
    monkeypatch.setattr(N, "corr_pyramid_layout", never)
    monkeypatch.setattr(raft, "_check_maps", lambda *args: (1, 16, 24))  # it refuses CPU images first; this test is about the check after it
    with pytest.raises(ValueError, match="16 x 24 give 2 x 3 feature maps, too small for 3 correlation levels.*avg_pool2d"):
        model(make_image(1, 1, 16, 24, 1), make_image(1, 1, 16, 24, 2))


# the walk of tests/args_walk.py (duck-typed tensors, a recording stand-in for the native library) over the two entries


def _walk(monkeypatch, spoil=None):
    from feature_tracker_amd import _native as N
    w = A.Walk(monkeypatch, spoil=spoil)
    monkeypatch.setattr(N, "corr_ondemand_layout", lambda B, C, H, W, levels: (B * C * 2 * H * W, [], []))
    return w


def _calls(w):
    from feature_tracker_amd import device as D
    return {"prepare": lambda: D.corr_ondemand_prepare_device(w.ctx, w.t("fmap0", "float32", 1, 4, 4, 6), w.t("fmap1", "float32", 1, 4, 4, 6), 1,
                                                              w.t("workspace", "float32", 192)),
            "lookup": lambda: D.corr_ondemand_lookup_device(w.ctx, w.t("workspace", "float32", 192), 4, 1, 1, w.t("coords", "float32", 1, 2, 4, 6),
                                                            w.t("out", "float32", 1, 9, 4, 6))}


@pytest.mark.parametrize("entry", ["prepare", "lookup"])
def test_device_entries_take_no_pointer_of_an_unchecked_argument(monkeypatch, entry):
    w = _walk(monkeypatch)
    _calls(w)[entry]()
    assert w.unchecked_reads == []
    assert w.lib.calls == [f"ftk_corr_ondemand_{entry}_device"]
    assert [f.name for f in w.made if f.reads != 1] == []


@pytest.mark.parametrize("entry", ["prepare", "lookup"])
@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("kind", ["dtype", "shape"])
def test_device_entries_stop_before_the_library(monkeypatch, entry, which, kind):
    """Each tensor of the call in turn made float64, or one element longer in its last dimension."""
    w = _walk(monkeypatch, spoil=(which, kind, A.one_column_more if kind == "shape" else None))
    with pytest.raises(ValueError):
        _calls(w)[entry]()
    assert w.lib.calls == [] and w.unchecked_reads == []


def test_lookup_entry_refuses_radius_and_coords_shape(monkeypatch):
    from feature_tracker_amd import device as D
    w = _walk(monkeypatch)
    with pytest.raises(ValueError, match="radius 65"):
        D.corr_ondemand_lookup_device(w.ctx, w.t("workspace", "float32", 192), 4, 1, 65, w.t("coords", "float32", 1, 2, 4, 6), w.t("out", "float32", 1, 9, 4, 6))
    with pytest.raises(ValueError, match=r"coords must be \[B, 2, H, W\]"):
        D.corr_ondemand_lookup_device(w.ctx, w.t("workspace", "float32", 192), 4, 1, 1, w.t("coords", "float32", 1, 3, 4, 6), w.t("out", "float32", 1, 9, 4, 6))
    assert w.lib.calls == []


# ---- the launch plan ----------------------------------------------------------------------------------------------------------------

# (B, C, H, W, levels, radius): the shapes tests/test_raft_corr_ondemand_gpu.py runs, and the production ones
GPU_SHAPES = [(5, 128, 8, 8, 3, 3), (1, 1, 17, 23, 3, 2), (3, 67, 19, 13, 3, 3), (2, 5, 33, 35, 5, 1), (1, 2, 9, 70, 2, 0), (1, 256, 12, 20, 3, 4),
              (1, 8, 4, 9, 2, 2), (1, 3, 20, 24, 2, 8), (1, 64, 48, 64, 3, 4), (1, 256, 55, 128, 4, 4), (1, 256, 135, 240, 4, 4)]


def plan(cases):
    assert os.path.exists(PLAN_CLI), "host layer not built (python -c 'import __graft_entry__ as g; g.build()')"
    text = "\n".join(" ".join(str(e) for e in c) for c in cases) + "\n"
    r = subprocess.run([PLAN_CLI], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        d = {}
        for kv in line.split():
            k, v = kv.split("=")
            d[k] = tuple(int(e) for e in v.split("x")) if "grid" in k or "block" in k else int(v) if v.lstrip("-").isdigit() else v
        out.append(d)
    assert len(out) == len(cases)
    return out


def cdiv(a, b):
    return -(-a // b)


def test_plan_at_the_gpu_shapes():
    from feature_tracker_amd import _native as N
    seen = set()
    for c, p in zip(GPU_SHAPES, plan(GPU_SHAPES)):
        B, C, H, W, L, r = c
        what = f"{c} -> {p}"
        assert p["refused"] == "none", what
        elements, offsets, dims = N.corr_ondemand_layout(B, C, H, W, L)
        assert p["elements"] == elements, what
        for l, (off, (h, w)) in enumerate(zip(offsets, dims)):
            pool_blocks = 0 if l == 0 else cdiv(B * C * h * w, 256)
            assert p[f"level{l}"] == f"{h}x{w}@{off}/{pool_blocks}", what
        # the window and its lattice: (2r + 2)^2 points while a wave's LDS share holds them, none above
        assert (p["side"], p["samples"], p["sample_passes"]) == (2 * r + 1, (2 * r + 1) ** 2, cdiv((2 * r + 1) ** 2, 64)), what
        if 2 * r + 2 <= 16:
            assert (p["lattice_side"], p["lattice_points"], p["lattice_passes"]) == (2 * r + 2, (2 * r + 2) ** 2, cdiv((2 * r + 2) ** 2, 64)), what
            assert p["lattice_points"] <= p["lattice_floats"], what
        else:
            assert (p["lattice_side"], p["lattice_points"], p["lattice_passes"]) == (0, 0, 0), what
        seen.add((p["lattice_side"] > 0, p["vector"], p["lattice_passes"]))
        assert p["vector"] == int(C % 4 == 0), what
        assert p["lds"] == 4 * 4 * p["lattice_floats"] <= 64 * 1024, what
        # one wave per (pixel, level): four pixels to a workgroup, every pixel owned once
        assert p["lookup_grid"] == (cdiv(H * W, 4), L, B) and p["lookup_block"] == (256,), what
        assert p["transpose_grid"] == (cdiv(H * W, 32), cdiv(C, 32), 2 * B) and p["transpose_block"] == (32, 8), what
    assert {s[0] for s in seen} == {True, False} and {s[1] for s in seen} == {0, 1} and {1, 2} <= {s[2] for s in seen}


def test_plan_alignment_and_refusals():
    got = plan([(1, 8, 4, 4, 1, 1, 0), (1, 8, 4, 4, 1, 1, 1), (1, 6, 4, 4, 1, 1, 1), (0, 8, 4, 4, 1, 1), (1, 0, 4, 4, 1, 1), (1, 8, 4, 4, 0, 1), (1, 8, 4, 4, 17, 1),
                (1, 8, 6, 9, 4, 1), (1, 8, 4, 4, 1, -1), (1, 8, 4, 4, 1, 65), (1, 8, 4, 4, 1, 64), (40000, 8, 4, 4, 1, 1), (1, 8, 4, 4, 1, 7), (1, 8, 4, 4, 1, 8),
                (2 ** 15, 2 ** 30, 2 ** 15, 2 ** 15, 1, 1)])
    assert [p["vector"] for p in got[:3]] == [0, 1, 0]
    assert [p["refused"] for p in got[3:]] == ["sizes", "channels", "levels", "levels", "empty_level", "radius", "radius", "none", "grid", "none", "none", "overflow"]
    assert got[7]["empty_level"] == 3
    assert got[10]["lattice_side"] == 0 and got[10]["samples"] == 129 ** 2
    assert got[12]["lattice_side"] == 16 and got[13]["lattice_side"] == 0  # the threshold between the two forms of the lookup
