"""What tests/test_raft_entries_guarded_gpu.py rests on, without a device:

 - every spec list of that file passes the argument checks of its entry: the same arenas built on CPU tensors, the entries run up to their
   native call over a recording stand-in of the library, and a written payload one element off is refused;
 - every shape list reaches the tails its comments claim, by the plan tools' geometry and the layouts;
 - the two correlation pyramids no other test builds (one level; 8 x 8 with 4 levels, whose last level is 1 x 1): the restatement against
   torch's own composition on the CPU, the NaNs at the same places;
 - a stand-in that stores whole tiles, a numpy writer into the arena's own buffer that ignores a tail, is named by ``check()`` with the right
   neighbour and offset, one row and one plane past the end: the bands are wide enough for these layouts.

The only damage done here is numpy indexing into the arena's own allocation."""
import types

import numpy as np
import pytest

from tests import args_walk as A
from tests import guarded as G
from tests import raft_corr_ondemand_ref as CO
from tests import raft_corr_ref as CR
from tests import test_raft_entries_guarded_gpu as E
from tests import test_superpoint_cpu as TS
from tests.test_raft_corr_cpu import LOOKUP_TOL, levels_np, torch_lookup, torch_pyramid

torch = pytest.importorskip("torch")

from feature_tracker_amd import _native as N  # noqa: E402
from feature_tracker_amd import device as D  # noqa: E402

HOST_ONLY = ("ftk_corr_pyramid_layout", "ftk_corr_ondemand_layout", "ftk_flow_warm_splits", "ftk_last_error")


class Recorder:
    """Stands where the loaded library stands: the host-only entries answer as the library does, every other one is recorded and
    answers FTK_OK; nothing is launched."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in HOST_ONLY:
            return getattr(self.real, name)
        if not name.startswith("ftk_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            return 0

        return entry


@pytest.fixture
def walk(monkeypatch):
    """The entries on CPU tensors: every check of dtype, shape, element count and stride is the real one, only where a tensor lives is not
    asked, and the library is the recorder."""
    recorder = Recorder(N.lib())
    stream = types.SimpleNamespace(cuda_stream=0)
    fake_torch = types.SimpleNamespace(cuda=types.SimpleNamespace(current_stream=lambda device=None: stream))
    monkeypatch.setattr(N, "lib", lambda: recorder)
    monkeypatch.setattr(D, "_torch", lambda: fake_torch)
    monkeypatch.setattr(D, "_device_complaint", lambda name, t, device_index: None)
    return types.SimpleNamespace(lib=recorder, ctx=types.SimpleNamespace(handle=None, device_index=None))


def _arena(specs, inputs):
    arena = E.make_arena(specs, inputs, G.ONES, "cpu")
    for name, _, shape, _ in specs:  # (a) and (e): exactly the spec's elements, on a 256-byte boundary
        assert tuple(arena[name].shape) == shape and arena[name].data_ptr() % G.ALIGN == 0 and arena[name].is_contiguous()
    return arena


def _one_off(specs, name):
    """The spec list with payload ``name`` one element shorter in its last dimension (longer where that is 1)."""
    out = []
    for n, dtype, shape, fill in specs:
        if n == name:
            shape = shape[:-1] + (shape[-1] - 1 if shape[-1] > 1 else 2,)
        out.append((n, dtype, shape, fill))
    return out


def _walk_entry(walk, specs, inputs, call, native, written):
    """``call(arena)`` passes every check and reaches exactly ``native``; with a written payload one element off it is refused before."""
    call(_arena(specs, inputs))
    assert walk.lib.calls == native, walk.lib.calls
    for name in written:
        del walk.lib.calls[:]
        spoiled = _one_off(specs, name)
        with pytest.raises(ValueError, match="must"):
            call(E.make_arena(spoiled, {k: v for k, v in inputs.items() if k != name}, G.ONES, "cpu"))
        assert walk.lib.calls == [], name
    del walk.lib.calls[:]


# ---- the spec lists against the entries' own checks ---------------------------------------------------------------------------------------------

def test_conv_specs_pass_the_entries_checks(walk):
    for k in range(len(E.CONV_CASES)):
        _walk_entry(walk, E.conv_specs(k), E.conv_case(k)[0], lambda a: E.conv_call(D, walk.ctx, a, k), ["ftk_conv2d_device"], ["out"])
    for k in range(len(E.STRIDED_CASES)):
        _walk_entry(walk, E.strided_specs(k), E.strided_case(k)[0], lambda a: E.strided_call(D, walk.ctx, a, k), ["ftk_conv2d_strided_device"], ["out"])
    for k in range(len(TS.POOL_CASES)):
        _walk_entry(walk, E.pool_specs(k), E.pool_case(k)[0], lambda a: E.pool_call(D, walk.ctx, a, k), ["ftk_conv2d_pool_device"], ["out"])
    for d, grid in E.NORMALISE_CASES:
        for x in E.normalise_inputs(d, grid):
            _walk_entry(walk, E.normalise_specs(d, grid), dict(x=x), lambda a: E.normalise_call(D, walk.ctx, a), ["ftk_channel_normalise_device"], ["out"])


def test_gru_specs_pass_the_entrys_checks(walk):
    four = ["ftk_sep_conv_gru_gates_device", "ftk_sep_conv_gru_blend_device"] * 2
    for k in range(len(E.GRU_CASES)):
        _walk_entry(walk, E.gru_specs(k), E.gru_case(k)[0], lambda a: E.gru_call(D, walk.ctx, a, k), four, list(E.GRU_SCRATCH) + ["out"])


def test_correlation_specs_pass_the_entries_checks(walk):
    for case in E.CORR_CASES:
        f0, f1, c = E.corr_case(case)
        B, C, H, W, L, r = E.corr_sizes(case)
        inputs = dict(fmap0=f0, fmap1=f1, coords=c)
        specs = E.corr_specs(case)
        sizes = {name: int(np.prod(shape)) for name, _, shape, _ in specs}
        K = (2 * r + 1) ** 2
        assert sizes["volume"] == B * H * W * sum(h * w for h, w in CR.layout(H, W, L))  # the layout's count, with no added term
        assert sizes["out_fused"] == sizes["out_per_level"] == B * L * K * H * W
        _walk_entry(walk, specs, inputs, lambda a: E.corr_build_call(D, walk.ctx, a, case), ["ftk_corr_pyramid_build_device"], ["volume"])
        for per_level in (False, True):
            _walk_entry(walk, specs, inputs, lambda a: E.corr_lookup_call(D, walk.ctx, a, case, per_level), ["ftk_corr_pyramid_lookup_device"],
                        ["volume", "out_per_level" if per_level else "out_fused"])
        specs = E.ondemand_specs(case)
        assert dict((s[0], int(np.prod(s[2]))) for s in specs)["workspace"] == B * C * (H * W + sum(h * w for h, w in CR.layout(H, W, L)))
        _walk_entry(walk, specs, inputs, lambda a: E.ondemand_prepare_call(D, walk.ctx, a, case), ["ftk_corr_ondemand_prepare_device"], ["workspace"])
        for per_level in (False, True):
            _walk_entry(walk, specs, inputs, lambda a: E.ondemand_lookup_call(D, walk.ctx, a, case, per_level), ["ftk_corr_ondemand_lookup_device"],
                        ["workspace", "out_per_level" if per_level else "out_fused"])


def test_flow_specs_pass_the_entries_checks(walk):
    for case in E.UPSAMPLE_CASES:
        flow, mask, _, _ = E.upsample_case(case)
        _walk_entry(walk, E.upsample_specs(case), dict(flow=flow, mask=mask), lambda a: E.upsample_call(D, walk.ctx, a, case), ["ftk_flow_upsample_device"], ["out"])
    for case in E.WARM_CASES:
        flow, _ = E.warm_case(*case)
        _, (H, W), B = case
        assert set(E.WARM_SPLITS) <= set(E.warm_splits(case)) and N.flow_warm_splits(B, H, W) in E.warm_splits(case)
        for splits in E.warm_splits(case):
            specs = E.warm_specs(case, splits)
            assert ("workspace" in [s[0] for s in specs]) == (splits > 1)
            if splits > 1:
                assert dict((s[0], s[2]) for s in specs)["workspace"] == (splits * B * H * W,)
            _walk_entry(walk, specs, dict(flow=flow), lambda a: E.warm_call(D, walk.ctx, a, case, splits), ["ftk_flow_warm_device"],
                        ["out"] + (["workspace"] if splits > 1 else []))
    for grid in E.POINT_GRIDS:
        for count in E.POINT_COUNTS:
            for n in range(2):
                inputs, image_size, mask_scale, _, _ = E.points_case(grid, count, n)
                for form in E.POINT_FORMS:
                    specs = E.points_specs(grid, count, form)
                    given = {name: a for name, a in inputs.items() if name in [s[0] for s in specs]}
                    written = ["cur_points", "status"] + (["fb_error2"] if form == "forward-backward" else [])
                    _walk_entry(walk, specs, given, lambda a: E.points_call(D, walk.ctx, a, form, image_size, mask_scale), ["ftk_flow_track_points_device"],
                                written)


# ---- the shape lists reach the tails ---------------------------------------------------------------------------------------------------------------

def _plans(tool, cases):
    return [{k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in p.items()} for p in A.run_plan_tool(A.plan_cli(tool), cases, timeout=120)]


def _crosses(split, chunk):
    """A part of the channel counts ``split`` begins and ends in different chunks."""
    edges = np.cumsum((0,) + tuple(split))
    return any(a // chunk != (b - 1) // chunk for a, b in zip(edges[:-1], edges[1:]))


def _tile_tails(plan, out_h, out_w):
    """(a last tile of pixels that is partial behind a whole one, a last workgroup with fewer rows than it computes)."""
    return (plan["tiles_x"] >= 2 and out_w % plan["tile_w"] != 0, plan["tiles_y"] >= 2 and out_h % plan["tile_h"] != 0)


def test_the_conv_shapes_reach_every_tail():
    from tests.test_update_block_gpu import CONV_SHAPES
    shapes = [c[0] for c in E.CONV_CASES]
    assert set(s for s, split in E.CONV_CASES if split is None) <= set(CONV_SHAPES)
    plans = _plans("raft_conv_plan_cli", [(Cout, Cin, ks, B, H, W) for Cin, Cout, ks, _, _, B, H, W in shapes])
    assert all(p["refused"] == "none" for p in plans)
    wide, short = set(), set()
    for (Cin, Cout, ks, _, _, B, H, W), p in zip(shapes, plans):
        x_tail, y_tail = _tile_tails(p, H, W)
        if x_tail:
            wide.add(p["wn"])
        if y_tail:
            short.add(p["wn"])
    assert wide == {4, 2, 1} and short >= {4, 2}  # (a workgroup of wn 1 has no row to lose)
    by_cout = {s[1]: p for s, p in zip(shapes, plans)}
    assert [(by_cout[m]["wm"], by_cout[m]["m_tiles"]) for m in (2, 33, 100)] == [(1, 1), (2, 2), (4, 4)] and all(m % 32 for m in (2, 33, 100))
    assert {ks for (Cin, _, ks, *_), p in zip(shapes, plans) if Cin % p["chunk"]} == {1, 3, 7}  # a partial last chunk at every kernel size
    assert any(s[5] == 2 for s in shapes) and {(1, 1), (2, 1)} <= {s[6:] for s in shapes}
    two = [(s, split, p) for (s, split), p in zip(E.CONV_CASES, plans) if split is not None]
    assert len(two) == 1 and len(two[0][1]) == 2 and _crosses(two[0][1], two[0][2]["chunk"])


def test_the_strided_shapes_reach_every_tail():
    from tests import test_raft_encoder_gpu as T
    cases = E.STRIDED_CASES
    plans = _plans("raft_conv_plan_cli", [(Cout, Cin, ks, 2, H, W, stride) for ks, Cin, Cout, stride, H, W, *_ in cases])
    assert all(p["refused"] == "none" for p in plans)
    stride1 = [(3, 9, 33, 5, 35), (1, 33, 100, 9, 67), (3, 9, 2, 9, 33), (7, 3, 40, 5, 35)]  # the list of its stride-1 test
    for (ks, Cin, Cout, stride, H, W, *_), p in zip(cases, plans):
        assert (p["out_h"], p["out_w"]) == (-(-H // stride), -(-W // stride))
        if stride == 2:
            assert (ks, Cin) in T.KERNELS and Cout in T.C_OUTS and H in T.HEIGHTS and W in T.WIDTHS
        else:
            assert (ks, Cin, Cout, H, W) in stride1
    s2 = [(c, p) for c, p in zip(cases, plans) if c[3] == 2]
    assert {c[0] for c, _ in s2} == {1, 3}
    wide = {p["wn"] for c, p in s2 if _tile_tails(p, p["out_h"], p["out_w"])[0]}
    short = {p["wn"] for c, p in s2 if _tile_tails(p, p["out_h"], p["out_w"])[1]}
    assert wide == {4, 2, 1} and short >= {4, 2}
    for ks in (1, 3):
        assert any(c[0] == ks and c[4] % 2 and c[5] % 2 for c, _ in s2), ks                    # odd H and W: the odd plane is the shorter one
        # W 65 / 66: a second tile of one output column, whose input column 64 is the image's last or last but one.  Kernel size 3 stages two
        # planes of 33 columns per row, so a 66th staged column exists; kernel size 1 stages the 32 even columns alone
        assert any(c[0] == ks and c[5] in (65, 66) and p["tiles_x"] == 2 and p["row"] == (66 if ks == 3 else 32) for c, p in s2), ks
    assert {c[5] for c, _ in s2} >= {65, 66} and {(c[4], c[5]) for c, _ in s2} >= {(1, 1), (2, 1)}
    assert {c[2] for c in cases} >= {2, 33, 100} and all(c[1] % p["chunk"] for c, p in zip(cases, plans))
    two = [(c, p) for c, p in zip(cases, plans) if c[8] is not None]
    assert len(two) == 1 and len(two[0][0][8]) == 2 and _crosses(two[0][0][8], two[0][1]["chunk"])
    s1 = {c[6] for c in cases if c[3] == 1}
    assert s1 >= {"residual", "normalise", "both"}
    for k, c in enumerate(cases):
        if c[6] in ("normalise", "both"):  # pixel values, as the encoders' first layer sees them
            x = np.concatenate([E.strided_case(k)[0][n] for n in E.strided_case(k)[1]], axis=1)
            assert x.min() >= 0 and x.max() <= 255 and (x == np.floor(x)).all() and x.max() > 100


def test_the_pooled_shapes_reach_every_tail():
    cases = TS.POOL_CASES
    plans = _plans("raft_conv_plan_cli", [(M, sum(channels), ks, B, H, W, 1, 1) for ks, _, channels, M, H, W, B in cases])
    assert all(p["refused"] == "none" and p["pool"] == 1 for p in plans)
    assert {(c[4], c[5]) for c in cases} >= {(2, 2), (3, 3), (5, 70), (9, 33)} and {c[3] for c in cases} >= {65, 130}
    for (ks, _, channels, M, H, W, B), p in zip(cases, plans):
        assert (p["out_h"], p["out_w"]) == (H // 2, W // 2)
        assert p["tiles_y"] * p["tile_h"] >= 2 * (H // 2) and p["tiles_x"] * p["tile_w"] >= 2 * (W // 2)
    # an odd size whose dropped last row / column lies in a tile that is computed: its pool is never stored
    assert any(c[4] % 2 and p["tiles_y"] * p["tile_h"] > c[4] - 1 for c, p in zip(cases, plans))
    assert any(c[5] % 2 and p["tiles_x"] * p["tile_w"] > c[5] - 1 for c, p in zip(cases, plans))
    assert any(p["tiles_x"] >= 2 and (c[5] // 2 * 2) % p["tile_w"] for c, p in zip(cases, plans))  # a partial last tile behind a whole one
    assert any((c[4] // 2 * 2) % p["tile_h"] for c, p in zip(cases, plans))  # a last workgroup with fewer rows than wn (2 x 2 and 3 x 3 at wn 4)
    assert any(c[4] % 2 and c[5] % 2 for c in cases) and any(c[6] == 2 for c in cases)
    assert {p["wn"] for p in plans} == {4, 2} and any(p["m_groups"] > 1 for p in plans)
    assert any(c[3] % 32 and sum(c[2]) % p["chunk"] for c, p in zip(cases, plans))
    assert any(len(c[2]) == 2 and _crosses(c[2], p["chunk"]) for c, p in zip(cases, plans))
    assert {1, 63, 64, 65} <= set(TS.NORMALISE_CHANNELS) and {(1, 1), (9, 33)} <= set(TS.NORMALISE_GRIDS)


def test_the_gru_shapes_reach_every_tail():
    from tests.test_sep_conv_gru_gpu import SHAPES
    shapes = [c[0] for c in E.GRU_CASES]
    assert set(s for s, split in E.GRU_CASES if split is None) <= set(SHAPES)
    assert {s[4:] for s in shapes} >= {(1, 1), (1, 7), (7, 1), (2, 131)}
    lines = [(Ch, Cx + Ch, ks, vertical, gates, B, H, W) for Cx, Ch, ks, B, H, W in shapes for vertical in (0, 1) for gates in (1, 0)]
    plans = _plans("sep_conv_gru_plan_cli", lines)
    assert all(p["refused"] == "none" for p in plans)
    tails = {(vertical, axis): set() for vertical in (0, 1) for axis in "xy"}
    for (Ch, Cin, ks, vertical, gates, B, H, W), p in zip(lines, plans):
        assert p["out_channels"] == (2 * Ch if gates else Ch)
        x_tail, y_tail = _tile_tails(p, H, W)
        if x_tail:
            tails[vertical, "x"].add(p["wn"])
        if y_tail:
            tails[vertical, "y"].add(p["wn"])
    # a strip of 32 wn pixels of a row in the horizontal pass, wn rows of 32 pixels in the vertical one: a partial last strip at every wn
    assert tails[0, "x"] == {4, 2, 1} and tails[1, "x"] == {4, 2, 1} and tails[1, "y"] >= {4, 2}
    assert any(p["out_channels"] % 32 for p in plans) and any(s[3] == 2 for s in shapes)
    (s, split), = [c for c in E.GRU_CASES if c[1] is not None]
    assert len(split) == 3 and _crosses(split, N.FTK_SEP_CONV_GRU_CHUNK) and (s[0] + s[1]) % N.FTK_SEP_CONV_GRU_CHUNK


def test_the_correlation_cases_reach_every_tail():
    sizes = [E.corr_sizes(c) for c in E.CORR_CASES]
    for HW_case in ((17, 23), (19, 13)):
        assert any((H, W) == HW_case and (H * W) % 32 and (H * W) % 128 and W % 16 and H % 8 for _, _, H, W, _, _ in sizes)
    # a partial q block of 8 x 16 in both axes, and at every pooled level of the build's epilogue an odd size whose last row or column is dropped
    B, C, H, W, L, r = 3, 67, 19, 13, 3, 3
    assert (B, C, H, W, L, r) in sizes and C % 2 == 1
    for case in ((1, 1, 17, 23, 3, 2), (3, 67, 19, 13, 3, 3)):
        dims = N.corr_pyramid_layout(case[0], case[2], case[3], case[4])[2]
        assert all(h % 2 or w % 2 for h, w in dims[:-1]), dims
    five = [s for s in sizes if s[4] == 5]
    assert five and all(N.corr_pyramid_layout(s[0], s[2], s[3], 5)[2][4][0] >= 1 for s in five)  # level 4 is corr_pool_kernel's
    assert E.CORR_ONE_LEVEL in sizes and E.CORR_ONE_LEVEL[4] == 1
    B, C, H, W, L, r = E.CORR_LAST_LEVEL_1X1
    assert E.CORR_LAST_LEVEL_1X1 in sizes and N.corr_pyramid_layout(B, H, W, L)[2][-1] == (1, 1)
    with pytest.raises(N.FtkError, match="avg_pool2d"):  # the smallest size before the refusal
        N.corr_pyramid_layout(B, H, W, L + 1)
    assert any(s[5] == 0 for s in sizes) and any(2 * s[5] + 1 >= max(s[2], s[3]) for s in sizes)  # r 0, and a window as wide as the map
    c = E.corr_case("hostile")[2]
    assert np.isnan(c).any() and np.isposinf(c).any() and np.isneginf(c).any() and (np.abs(c[np.isfinite(c)]) >= 1e30).any() and (c == 2.0 ** 31).any()
    for case in E.CORR_CASES:  # nothing here needs the workload's sizes
        B, C, H, W, L, r = E.corr_sizes(case)
        assert max(H, W, C) < 140 and 4 * N.corr_pyramid_layout(B, H, W, L)[0] < 16 << 20


def test_the_flow_cases_reach_every_tail():
    from tests.test_flow_upsample_gpu import SHAPES
    T = N.FTK_FLOW_UPSAMPLE_TILE
    ups = [c[:3] for c in E.UPSAMPLE_CASES if c != "hostile"]
    assert set(ups) <= set(SHAPES) and {(1, 1, 1), (1, 2, T - 1), (1, 2, T), (1, 2, T + 1), (2, 5, 2 * T + 3)} <= set(ups)
    flow, mask, want, _ = E.upsample_case("hostile")
    assert np.isnan(want).any() and not np.isnan(want).all()
    tile = N.FTK_FLOW_WARM_TILE
    warm = [(H * W, H, W, B) for _, (H, W), B in E.WARM_CASES]
    assert {1, tile + 1} <= {w[0] for w in warm} and any(w[1] == 1 for w in warm) and any(w[2] == 1 for w in warm)
    assert any(w[0] < tile for w in warm) and any(w[0] > 2 * tile and N.flow_warm_splits(w[3], w[1], w[2]) > 1 for w in warm) and any(w[3] == 3 for w in warm)
    hostile, _ = E.warm_case("hostile", (33, 65), 3)
    assert np.isnan(hostile).any() and np.isinf(hostile).any()
    P = N.FTK_FLOW_POINTS_TILE
    assert E.POINT_COUNTS == (1, P - 1, P, P + 1) and {(1, 1, 1), (1, 2, 33)} <= set(E.POINT_GRIDS)
    for grid in E.POINT_GRIDS:
        for n in range(2):
            inputs, (rows, cols), _, both, forward = E.points_case(grid, P - 1, n)
            p = inputs["points"]
            with np.errstate(invalid="ignore"):
                outside = (p[..., 0] < 0) | (p[..., 0] > cols - 1) | (p[..., 1] < 0) | (p[..., 1] > rows - 1)
            assert np.isnan(p).any() and np.isinf(p).any() and outside.any() and not outside.all()
            assert E.FP.OUTSIDE in forward[1] and both[2] is not None and forward[2] is None


# ---- the two pyramids no other test builds: the restatement against torch on the CPU --------------------------------------------------------------

@pytest.mark.parametrize("case", [E.CORR_ONE_LEVEL, E.CORR_LAST_LEVEL_1X1], ids=str)
def test_the_new_pyramids_against_torch(case):
    """One level: no pooled level exists.  A last level of 1 x 1: correlation_volumes.py divides by w - 1 = 0 and h - 1 = 0, the normalised
    coordinate is +-inf or NaN, grid_sample's unnormalise multiplies it by (size - 1) / 2 = 0, and every sample of that level is NaN, in
    torch's composition and in the restatement alike; the levels before it hold no NaN."""
    B, C, H, W, L, r = case
    f0, f1, c = (torch.from_numpy(a.copy()) for a in E.corr_case(case))
    pyr = torch_pyramid(f0, f1, L)
    assert [tuple(p.shape[-2:]) for p in pyr] == N.corr_pyramid_layout(B, H, W, L)[2]
    for l in range(1, L):  # the pools, from torch's own level before
        assert CR.same(CR.pool(pyr[l - 1][:, 0].numpy()), pyr[l][:, 0].numpy()), l
    ref = torch_lookup(pyr, c, r).numpy()
    mine = CR.lookup(levels_np(pyr), c.numpy(), r)
    K = (2 * r + 1) ** 2
    assert np.array_equal(np.isnan(mine), np.isnan(ref))
    nan_levels = [bool(np.isnan(ref[:, l * K:(l + 1) * K]).all()) for l in range(L)]
    assert nan_levels == [dims == (1, 1) for dims in N.corr_pyramid_layout(B, H, W, L)[2]] and not np.isnan(ref[:, :(L - 1) * K or K]).any()
    ok = ~np.isnan(ref)
    assert np.abs(mine[ok] - ref[ok]).max() <= LOOKUP_TOL * max(float(p.abs().max()) for p in pyr)
    # what the device is held to: the restatement from its own build, and the on-demand restatement, NaN where torch is NaN
    levels, want = E.corr_want(case)
    assert np.array_equal(np.isnan(want), np.isnan(ref)) and np.array_equal(np.isnan(E.ondemand_want(case)), np.isnan(ref))
    assert CR.same(E.ondemand_want(case)[:, :K], want[:, :K])  # level 0 is the same arithmetic


# ---- a writer of whole tiles is named by check() -----------------------------------------------------------------------------------------------------

def store_whole_tiles(arena, name, shape, axis, tile):
    """What a kernel without a tail guard on ``axis`` stores: every element of ``shape`` with that extent rounded up to ``tile``, at the
    address the true strides give.  A numpy write into the arena's own buffer.  Returns the bytes that lie past the payload."""
    a, b = arena.span(name)
    padded = list(shape)
    padded[axis] = -(-shape[axis] // tile) * tile
    strides = np.cumprod((1,) + tuple(shape[:0:-1]))[::-1]
    offsets = (np.indices(padded).reshape(len(shape), -1) * strides[:, None]).sum(0)
    raw = arena.buf.numpy()
    raw[a:a + 4 * (int(offsets.max()) + 1)].view(np.float32)[offsets] = 1.0
    return 4 * (int(offsets.max()) + 1) - (b - a)


def _named(arena, before, after, past):
    with pytest.raises(G.GuardDamaged) as e:
        arena.check()
    d = e.value
    assert (d.before, d.after, d.past_before, d.damaged, d.last - d.first + 1) == (before, after, 0, past, past), str(d)
    assert d.first == arena.span(before)[1] and d.last < (arena.span(after)[0] if after is not None else arena.total)
    assert d.ahead_of_after >= 1


def test_a_writer_of_whole_tiles_is_named_with_its_neighbour_and_offset():
    # conv2d_kernel's layout: a workgroup of wn 4 rows without `py >= OH` stores one row of 35 pixels past the end
    k = next(i for i, (s, _) in enumerate(E.CONV_CASES) if s[1:3] == (16, 3) and s[6:] == (9, 35))
    (Cin, Cout, ks, _, _, B, H, W), _ = E.CONV_CASES[k]
    specs = E.conv_specs(k)
    assert [s[0] for s in specs][-2:] == ["bias", "out"]
    arena = E.make_arena(specs, E.conv_case(k)[0], G.ZEROS, "cpu")
    arena.check()
    past = store_whole_tiles(arena, "out", (B, Cout, H, W), 2, 4)
    assert past == 3 * W * 4  # rows 9, 10 and 11 of the last plane
    _named(arena, "out", None, past)
    # without `co < Cout`: 100 channels stored as 128, 28 planes of 5 x 131 past the end, in front of the next payload
    k = next(i for i, (s, _) in enumerate(E.CONV_CASES) if s[:3] == (6, 100, 3))
    (Cin, Cout, ks, _, _, B, H, W), _ = E.CONV_CASES[k]
    specs = [s for s in E.conv_specs(k) if s[0] != "out"]
    specs.insert(1, E._spec("out", (B, Cout, H, W)))  # (an output in the middle of the arena: the band is the next payload's too)
    arena = E.make_arena(specs, E.conv_case(k)[0], G.ONES, "cpu")
    past = store_whole_tiles(arena, "out", (B, Cout, H, W), 1, 32)
    assert past == 28 * H * W * 4
    _named(arena, "out", specs[2][0], past)
    # the pooled epilogue without `oy >= PH`: the dropped row of a 5 x 70 input stored as a third row of 35
    k = next(i for i, c in enumerate(TS.POOL_CASES) if c[3:] == (130, 5, 70, 1))
    arena = E.make_arena(E.pool_specs(k), E.pool_case(k)[0], G.ZEROS, "cpu")
    past = store_whole_tiles(arena, "out", (1, 130, 2, 35), 2, 4)
    assert past == 2 * 35 * 4
    _named(arena, "out", None, past)
    # corr_build_kernel without `y3 < level_h[3]`, and the lookup without `pix >= HW`: one plane of the last level, one pixel row of K values
    case = (2, 5, 33, 35, 5, 1)
    B, C, H, W, L, r = case
    elements, offsets, dims = N.corr_pyramid_layout(B, H, W, L)
    f0, f1, c = E.corr_case(case)
    arena = E.make_arena(E.corr_specs(case), dict(fmap0=f0, fmap1=f1, coords=c), G.ONES, "cpu")
    n, (h, w) = B * H * W, dims[-1]
    assert elements - offsets[-1] == n * h * w
    raw = arena.buf.numpy()
    a, b = arena.span("volume")
    raw[a + 4 * offsets[-1]:a + 4 * (offsets[-1] + (n + 1) * h * w)].view(np.float32)[:] = 1.0  # n + 1 slabs of the last level
    _named(arena, "volume", "coords", h * w * 4)
    arena = E.make_arena(E.corr_specs(case), dict(fmap0=f0, fmap1=f1, coords=c), G.ONES, "cpu")
    K = (2 * r + 1) ** 2
    past = store_whole_tiles(arena, "out_per_level", (L, B, H * W, K), 2, 256)
    assert past == (-(H * W) % 256) * K * 4
    _named(arena, "out_per_level", None, past)
    # every band is at least as wide as the payload in front of it (up to 1 MiB): a whole plane past any of these tensors ends in a band
    for name, (a, b) in arena.spans.items():
        following = [s[0] for s in arena.spans.values() if s[0] >= b]
        assert (min(following) if following else arena.total) - b >= min(b - a, G.MAX_GUARD), name
