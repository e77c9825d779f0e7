"""The device entries of the RAFT and SuperPoint family, held to their tensors on guarded memory (tests/guarded.py): ``conv2d_device``,
``conv2d_strided_device``, ``conv2d_pool_device``, ``channel_normalise_device``, ``sep_conv_gru_device``, ``corr_pyramid_build_device`` and
``corr_pyramid_lookup_device``, ``corr_ondemand_prepare_device`` and ``corr_ondemand_lookup_device``, ``flow_upsample_device``,
``flow_warm_device`` and ``flow_track_points_device``, called directly, not through the classes:

 (a) every tensor a call may write (outputs, the GRU's ``z`` / ``rh`` / ``mid``, the correlation volume, the workspaces) is a guarded payload
     of exactly its documented shape or element count: ``corr_pyramid_layout``, ``corr_ondemand_layout`` and ``splits * B * H * W`` words,
     with no added term;
 (b) every tensor a call only reads (parts, ``h``, feature maps, coordinates, residual, mask, flow, points, packed weights, biases) is a
     payload too, and holds its bytes unchanged after the call;
 (c) every call is made twice on fresh arenas, all payloads 0x00 and all payloads 0xFF (NaN floats), and both results equal the scalar
     restatement of that operator bit for bit, any NaN equal to any NaN: nothing depends on what a buffer held before.  The buffers that
     have no restatement of their own (``z``, ``rh``, ``mid``, the on-demand workspace) hold the same bytes after both runs;
 (d) no guard band is written;
 (e) every payload starts 256-byte aligned, as a block of torch's allocator does.

The tile kernels compute whole tiles and drop what lies outside the tensor, so the shapes are the smallest of each operator's own lists
at which every axis of a tile has a tail; tests/test_raft_entries_guarded_cpu.py holds the lists to that, and runs every spec list below
through the entries' argument checks without a device.  No kernel is run out of bounds here.

The case lists, spec lists and calls below take the device as an argument: the CPU file builds the same arenas on CPU tensors."""
import functools

import numpy as np
import pytest

from tests import flow_points_ref as FP
from tests import flow_upsample_ref as FU
from tests import flow_warm_ref as FW
from tests import guarded as G
from tests import raft_conv_ref as RC
from tests import raft_corr_ondemand_ref as CO
from tests import raft_corr_ref as CR
from tests import raft_encoder_ref as RE
from tests import sep_conv_gru_ref as SG
from tests import superpoint_ref as SP
from tests import test_superpoint_cpu as TS
from tests.test_flow_points_cpu import GRIDS as POINT_GRIDS
from tests.test_flow_points_cpu import fields, image_sizes, point_set
from tests.test_flow_upsample_cpu import hostile_inputs, inputs as upsample_inputs
from tests.test_flow_warm_gpu import case as warm_case
from tests.test_raft_corr_gpu import coords_for, features, hostile_case
from tests.test_raft_encoder_gpu import make_layer
from tests.test_sep_conv_gru_cpu import make_inputs as gru_inputs
from tests.test_sep_conv_gru_cpu import make_state as gru_state
from tests.test_update_block_gpu import make_conv

pytestmark = pytest.mark.gpu

FILLS = (G.ZEROS, G.ONES)
F32 = "float32"


def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _f32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)


def _spec(name, array_or_shape, dtype=F32):
    shape = array_or_shape.shape if hasattr(array_or_shape, "shape") else array_or_shape
    return (name, dtype, tuple(int(e) for e in shape), 0)


def _pack_conv(weight):
    """The packed matrix the classes hand to the conv entries, made on the host by the package's own packer."""
    import torch
    from feature_tracker_amd import raft
    return raft._pack_conv(torch.from_numpy(np.array(weight, copy=True))).numpy()


def make_arena(specs, inputs, fill, device="cuda"):
    arena = G.Arena(specs, device, fill=fill)
    for name, array in inputs.items():
        arena.put(name, array)
    return arena


def _ctx(arena):
    from feature_tracker_amd import raft
    return raft._device_context(arena.buf)


def _finish(arena, inputs):
    """(d) and (b) after the call: one synchronisation, one copy of the arena, every guard intact, every input as it was."""
    import torch
    torch.cuda.synchronize()
    host = arena.check()
    for name, array in inputs.items():
        assert arena.payload_bytes(name, host).tobytes() == np.ascontiguousarray(array).tobytes(), f"the call changed its input {name}"
    return host


def _np(arena, name):
    return arena[name].cpu().numpy()


def _where(got, want):
    return np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5].tolist()


def _split(x, split):
    """``x`` [B, C, H, W] as contiguous channel parts of the counts ``split`` (None: one part)."""
    if split is None:
        return (x,)
    assert sum(split) == x.shape[1]
    edges = np.cumsum((0,) + tuple(split))
    return tuple(np.ascontiguousarray(x[:, a:b]) for a, b in zip(edges[:-1], edges[1:]))


# ---- conv2d_device -------------------------------------------------------------------------------------------------------------------------
# ((C_in, C_out, kernel_size, relu, scale, B, H, W) of tests/test_update_block_gpu.py's CONV_SHAPES, the channel counts of the parts or None)
CONV_CASES = [
    ((6, 16, 3, True, 1.0, 1, 9, 35), None),     # wn 4: 35 = 32 + 3 pixels, 9 = 2 * 4 + 1 rows
    ((6, 48, 3, True, 1.0, 1, 5, 67), None),     # wn 2: 67 = 2 * 32 + 3, 5 = 2 * 2 + 1
    ((6, 100, 3, True, 1.0, 1, 5, 131), None),   # wn 1, wm 4 with an idle wave: 100 = 3 * 32 + 4 channels
    ((2, 100, 7, False, 1.0, 1, 5, 131), None),  # the same tiles under the 7 x 7 halo
    ((16, 2, 3, False, 1.0, 1, 4, 5), None),     # 2 output channels
    ((5, 33, 3, True, 1.0, 1, 4, 5), None),      # 33: one channel in the second tile
    ((131, 8, 3, True, 1.0, 1, 3, 4), None),     # a partial last chunk: 131 = 16 * 8 + 3
    ((33, 8, 1, True, 1.0, 1, 3, 4), None),      # 33 = 32 + 1
    ((3, 8, 7, False, 1.0, 1, 5, 6), None),      # 3 = 2 + 1
    ((10, 40, 3, True, 1.0, 2, 5, 9), None),     # B 2
    ((9, 8, 3, True, 1.0, 1, 1, 1), None),       # 1 x 1: smaller than the halo
    ((9, 40, 3, True, 1.0, 1, 2, 1), None),      # 2 x 1
    ((2, 8, 7, True, 1.0, 1, 1, 1), None),
    ((35, 40, 3, True, 1.0, 2, 5, 37), (3, 32)),  # two parts, the second across the chunk boundaries at 8, 16, 24 and 32
]


@functools.lru_cache(maxsize=None)
def conv_case(k):
    """(inputs by payload name, names of the parts, the restatement's output) of CONV_CASES[k]."""
    (Cin, Cout, ks, relu, scale, B, H, W), split = CONV_CASES[k]
    x, w, b = make_conv(Cin, Cout, ks, B, H, W, 11 if split is None else 12)
    parts = _split(x, split)
    inputs = {f"parts{i}": p for i, p in enumerate(parts)}
    inputs.update(packed_weights=_pack_conv(w), bias=b)
    want = RC.conv2d(x, w, b, relu, scale)
    _readonly(want, *inputs.values())
    return inputs, [f"parts{i}" for i in range(len(parts))], want


def conv_specs(k):
    (_, Cout, _, _, _, B, H, W), _ = CONV_CASES[k]
    inputs, _, _ = conv_case(k)
    return [_spec(n, a) for n, a in inputs.items()] + [_spec("out", (B, Cout, H, W))]


def conv_call(D, ctx, arena, k):
    (_, _, ks, relu, scale, _, _, _), _ = CONV_CASES[k]
    _, part_names, _ = conv_case(k)
    D.conv2d_device(ctx, [arena[n] for n in part_names], arena["packed_weights"], arena["bias"], ks, relu, scale, arena["out"])


@pytest.mark.parametrize("k", range(len(CONV_CASES)), ids=[str(c) for c in CONV_CASES])
def test_conv2d_on_guarded_memory(ftk, k):
    from feature_tracker_amd import device as D
    inputs, _, want = conv_case(k)
    for fill in FILLS:
        arena = make_arena(conv_specs(k), inputs, fill)
        conv_call(D, _ctx(arena), arena, k)
        _finish(arena, inputs)
        got = _np(arena, "out")
        assert RC.same(got, want), (hex(fill), _where(got, want))


# ---- conv2d_strided_device -----------------------------------------------------------------------------------------------------------------
# (kernel_size, C_in, C_out, stride, H, W, epilogue, relu, parts), B 2.  The kernel sizes, channel counts, heights and widths are those of
# tests/test_raft_encoder_gpu.py's lists; "normalise" feeds pixel values 0 .. 255, as its test does.
STRIDED_CASES = [
    (3, 9, 2, 2, 9, 65, "residual", True, None),      # wn 4: out 5 x 33, odd H and W, the odd staging plane one column shorter
    (1, 33, 33, 2, 5, 66, "plain", False, None),      # wn 2: out 3 x 33, the 66th staged column exists
    (3, 9, 100, 2, 3, 129, "residual", False, None),  # wn 1: out 2 x 65
    (1, 33, 100, 2, 9, 65, "plain", True, None),
    (3, 9, 40, 2, 1, 1, "residual", True, None),      # 1 x 1 and 2 x 1: smaller than the halo
    (1, 33, 33, 2, 2, 1, "plain", True, None),
    (3, 9, 33, 2, 5, 66, "residual", True, (3, 6)),   # two parts, the second across the chunk boundary at 8
    (3, 9, 33, 1, 5, 35, "residual", True, None),
    (3, 9, 33, 1, 5, 35, "normalise", True, None),
    (1, 33, 100, 1, 9, 67, "both", True, None),
    (3, 9, 2, 1, 9, 33, "residual", False, None),
    (7, 3, 40, 1, 5, 35, "normalise", True, None),
    (7, 3, 40, 1, 5, 35, "residual", True, None),
]


@functools.lru_cache(maxsize=None)
def strided_case(k):
    ks, Cin, Cout, stride, H, W, epilogue, relu, split = STRIDED_CASES[k]
    x, w, b, res = make_layer(Cin, Cout, ks, stride, 2, H, W, 7 if stride == 1 else 100 + k)
    normalise, with_res = epilogue in ("normalise", "both"), epilogue in ("residual", "both")
    if normalise:
        x = (np.floor(np.abs(x) * 100) % 256).astype(np.float32)
    parts = _split(x, split)
    inputs = {f"parts{i}": p for i, p in enumerate(parts)}
    inputs.update(packed_weights=_pack_conv(w), bias=b)
    if with_res:
        inputs["residual"] = res
    want = RE.conv2d(x, w, b, stride, res if with_res else None, relu, 1.0, normalise)
    _readonly(want, *inputs.values())
    return inputs, [f"parts{i}" for i in range(len(parts))], want


def strided_specs(k):
    inputs, _, want = strided_case(k)
    ks, Cin, Cout, stride, H, W = STRIDED_CASES[k][:6]
    return [_spec(n, a) for n, a in inputs.items()] + [_spec("out", (2, Cout, -(-H // stride), -(-W // stride)))]


def strided_call(D, ctx, arena, k):
    ks, _, _, stride, _, _, epilogue, relu, _ = STRIDED_CASES[k]
    _, part_names, _ = strided_case(k)
    D.conv2d_strided_device(ctx, [arena[n] for n in part_names], arena["packed_weights"], arena["bias"], ks, stride, relu, 1.0,
                            arena["residual"] if epilogue in ("residual", "both") else None, epilogue in ("normalise", "both"), arena["out"])


@pytest.mark.parametrize("k", range(len(STRIDED_CASES)), ids=[str(c) for c in STRIDED_CASES])
def test_conv2d_strided_on_guarded_memory(ftk, k):
    from feature_tracker_amd import device as D
    inputs, _, want = strided_case(k)
    for fill in FILLS:
        arena = make_arena(strided_specs(k), inputs, fill)
        strided_call(D, _ctx(arena), arena, k)
        _finish(arena, inputs)
        got = _np(arena, "out")
        assert RE.same(got, want), (hex(fill), _where(got, want))


# ---- conv2d_pool_device and channel_normalise_device ----------------------------------------------------------------------------------------
# every case of tests/test_superpoint_cpu.py's POOL_CASES: they are the small ones (2 x 2, odd sizes whose last row and column are computed
# and never stored, 65 and 130 output channels, two parts of which one crosses the chunk boundary at 8)

@functools.lru_cache(maxsize=None)
def pool_case(k):
    relu = TS.POOL_CASES[k][1]
    parts, weight, bias = TS.pool_case(k)
    inputs = {f"parts{i}": p for i, p in enumerate(parts)}
    inputs.update(packed_weights=_pack_conv(weight), bias=bias)
    want = SP.conv2d_pool(parts, weight, bias, relu)
    _readonly(want, inputs["packed_weights"])
    return inputs, [f"parts{i}" for i in range(len(parts))], want


def pool_specs(k):
    _, _, _, M, H, W, B = TS.POOL_CASES[k]
    inputs, _, _ = pool_case(k)
    return [_spec(n, a) for n, a in inputs.items()] + [_spec("out", (B, M, H // 2, W // 2))]


def pool_call(D, ctx, arena, k):
    ks, relu = TS.POOL_CASES[k][:2]
    _, part_names, _ = pool_case(k)
    D.conv2d_pool_device(ctx, [arena[n] for n in part_names], arena["packed_weights"], arena["bias"], ks, relu, arena["out"])


@pytest.mark.parametrize("k", range(len(TS.POOL_CASES)), ids=[str(c) for c in TS.POOL_CASES])
def test_conv2d_pool_on_guarded_memory(ftk, k):
    from feature_tracker_amd import device as D
    inputs, _, want = pool_case(k)
    for fill in FILLS:
        arena = make_arena(pool_specs(k), inputs, fill)
        pool_call(D, _ctx(arena), arena, k)
        _finish(arena, inputs)
        got = _np(arena, "out")
        assert SP.same(got, want), (hex(fill), _where(got, want))


NORMALISE_CASES = [(d, grid) for d in TS.NORMALISE_CHANNELS for grid in TS.NORMALISE_GRIDS]


def normalise_inputs(d, grid):
    """The seeded map of that size; at one cell also the all-zero and the all-NaN cell, for which the map has no room."""
    xs = [TS.normalise_case(d, *grid)]
    if grid == (1, 1):
        xs += list(_readonly(np.zeros((d, 1, 1), np.float32), np.full((d, 1, 1), np.nan, np.float32)))
    return xs


def normalise_specs(d, grid):
    return [_spec("x", (d,) + tuple(grid)), _spec("out", tuple(grid) + (d,))]


def normalise_call(D, ctx, arena):
    D.channel_normalise_device(ctx, arena["x"], arena["out"])


@pytest.mark.parametrize("d", TS.NORMALISE_CHANNELS)
def test_channel_normalise_on_guarded_memory(ftk, d):
    from feature_tracker_amd import device as D
    for grid in TS.NORMALISE_GRIDS:
        for x in normalise_inputs(d, grid):
            want = SP.channel_normalise(x)
            for fill in FILLS:
                arena = make_arena(normalise_specs(d, grid), dict(x=x), fill)
                normalise_call(D, _ctx(arena), arena)
                _finish(arena, dict(x=x))
                got = _np(arena, "out")
                assert SP.same(got, want), (grid, hex(fill), _where(got, want))


# ---- sep_conv_gru_device -------------------------------------------------------------------------------------------------------------------
# ((x_channels, h_channels, kernel_size, B, H, W) of tests/test_sep_conv_gru_gpu.py's SHAPES, the channel counts of the parts or None)
GRU_CASES = [
    ((3, 16, 5, 1, 1, 1), None), ((3, 16, 3, 1, 1, 7), None), ((3, 16, 5, 1, 7, 1), None), ((4, 16, 3, 1, 2, 131), None),  # narrower / shorter than the kernel
    ((3, 16, 5, 1, 9, 133), None),   # wn 4: 133 = 128 + 5 pixels of a strip, 9 = 2 * 4 + 1 rows
    ((3, 48, 3, 1, 7, 67), None),    # wn 2
    ((6, 100, 5, 2, 3, 35), None),   # wn 1, B 2, 100 = 3 * 32 + 4 channels
    ((2, 33, 5, 1, 4, 5), None),     # 33 (66 stacked) output channels
    ((35, 40, 5, 2, 5, 37), (3, 30, 2)),  # the three parts of its test: the second crosses the chunk boundaries at 16 and 32
]
GRU_SCRATCH = ("z", "rh", "mid")


@functools.lru_cache(maxsize=None)
def gru_case(k):
    import feature_tracker_amd as F
    (Cx, Ch, ks, B, H, W), split = GRU_CASES[k]
    seed = 11 if split is None else 12
    state = gru_state(Cx, Ch, ks, seed)
    x, h = (t.numpy() for t in gru_inputs(Cx, Ch, B, H, W, seed))
    parts = _split(x, split)
    inputs = {f"x{i}": p for i, p in enumerate(parts)}
    inputs["h"] = h
    packed = F.SepConvGru.from_state_dict(state)._packed  # the class's own packing, on the host
    inputs.update({key: packed[key].numpy() for key in packed_keys()})
    want = SG.forward(x, h, SG.weights_of(state))
    _readonly(want, *inputs.values())
    return inputs, [f"x{i}" for i in range(len(parts))], want


def packed_keys():
    from feature_tracker_amd._device_sep_conv_gru import PACKED_KEYS as keys
    return keys


def gru_specs(k):
    (_, Ch, _, B, H, W), _ = GRU_CASES[k]
    inputs, _, _ = gru_case(k)
    return [_spec(n, a) for n, a in inputs.items()] + [_spec(n, (B, Ch, H, W)) for n in GRU_SCRATCH + ("out",)]


def gru_call(D, ctx, arena, k):
    ks = GRU_CASES[k][0][2]
    _, part_names, _ = gru_case(k)
    D.sep_conv_gru_device(ctx, [arena[n] for n in part_names], arena["h"], {key: arena[key] for key in packed_keys()}, ks, arena["z"], arena["rh"],
                          arena["mid"], arena["out"])


@pytest.mark.parametrize("k", range(len(GRU_CASES)), ids=[str(c) for c in GRU_CASES])
def test_sep_conv_gru_on_guarded_memory(ftk, k):
    from feature_tracker_amd import device as D
    inputs, _, want = gru_case(k)
    scratch = []
    for fill in FILLS:
        arena = make_arena(gru_specs(k), inputs, fill)
        gru_call(D, _ctx(arena), arena, k)
        host = _finish(arena, inputs)
        got = _np(arena, "out")
        assert SG.same(got, want), (hex(fill), _where(got, want))
        scratch.append({n: arena.payload_bytes(n, host).tobytes() for n in GRU_SCRATCH})
    for n in GRU_SCRATCH:  # every element of the buffers in between is written before it is read: the same bytes from zeros and from NaNs
        assert scratch[0][n] == scratch[1][n], n


# ---- the correlation pyramid and the on-demand correlation ------------------------------------------------------------------------------------
# (B, C, H, W, levels, radius): the odd sizes of tests/test_raft_corr_gpu.py (HW no multiple of 32 or 128, W no multiple of 16, H no multiple of
# 8, odd level sizes whose last row and column every pool drops, C 1 / 67 / 5, B 3, five levels, r 0), its hostile coordinates, a window wider
# than the map, and two pyramids no other test builds: one level, and 8 x 8 with 4 levels, whose last level is 1 x 1
CORR_CASES = [(1, 1, 17, 23, 3, 2), (3, 67, 19, 13, 3, 3), (2, 5, 33, 35, 5, 1), (1, 2, 9, 70, 2, 0), (1, 1, 17, 23, 3, 11), (2, 3, 9, 11, 1, 2),
              (1, 4, 8, 8, 4, 1), "hostile"]
CORR_ONE_LEVEL, CORR_LAST_LEVEL_1X1 = (2, 3, 9, 11, 1, 2), (1, 4, 8, 8, 4, 1)


def corr_sizes(case):
    return (1, 8, 16, 24, 3, 3) if case == "hostile" else case


@functools.lru_cache(maxsize=None)
def corr_case(case):
    """(fmap0, fmap1, coords) as float32 arrays, seeded as tests/test_raft_corr_gpu.py seeds them."""
    if case == "hostile":
        f0, f1, c = hostile_case()
    else:
        B, C, H, W, L, r = case
        f0, f1 = features(H * W + C, B, C, H, W)
        c = coords_for(B * 7 + C, B, H, W)
    return _readonly(*(t.numpy().copy() for t in (f0, f1, c)))


@functools.lru_cache(maxsize=None)
def corr_want(case):
    """(the restatement's levels, its lookup [B, L * K, H, W])."""
    f0, f1, c = corr_case(case)
    _, _, _, _, L, r = corr_sizes(case)
    levels = CR.build(f0, f1, L)
    return levels, CR.lookup(levels, c, r)


@functools.lru_cache(maxsize=None)
def ondemand_want(case):
    f0, f1, c = corr_case(case)
    _, _, _, _, L, r = corr_sizes(case)
    return CO.lookup(f0, f1, L, c, r)


def per_level_form(fused, L, K):
    """[B, L * K, H, W] as the ``per_level`` layout: ``L`` consecutive [B, H, W, K] blocks."""
    return np.stack([np.moveaxis(fused[:, l * K:(l + 1) * K], 1, -1) for l in range(L)])


def _lookup_specs(case):
    B, _, H, W, L, r = corr_sizes(case)
    K = (2 * r + 1) ** 2
    return [_spec("coords", (B, 2, H, W)), _spec("out_fused", (B, L * K, H, W)), _spec("out_per_level", (L, B, H, W, K))]


def corr_specs(case):
    from feature_tracker_amd import _native as N
    B, C, H, W, L, _ = corr_sizes(case)
    return [_spec("fmap0", (B, C, H, W)), _spec("fmap1", (B, C, H, W)), _spec("volume", (N.corr_pyramid_layout(B, H, W, L)[0],))] + _lookup_specs(case)


def ondemand_specs(case):
    from feature_tracker_amd import _native as N
    B, C, H, W, L, _ = corr_sizes(case)
    return [_spec("fmap0", (B, C, H, W)), _spec("fmap1", (B, C, H, W)), _spec("workspace", (N.corr_ondemand_layout(B, C, H, W, L)[0],))] + _lookup_specs(case)


def corr_build_call(D, ctx, arena, case):
    D.corr_pyramid_build_device(ctx, arena["fmap0"], arena["fmap1"], corr_sizes(case)[4], arena["volume"])


def corr_lookup_call(D, ctx, arena, case, per_level):
    _, _, _, _, L, r = corr_sizes(case)
    D.corr_pyramid_lookup_device(ctx, arena["volume"], L, r, arena["coords"], arena["out_per_level" if per_level else "out_fused"], per_level=per_level)


def ondemand_prepare_call(D, ctx, arena, case):
    D.corr_ondemand_prepare_device(ctx, arena["fmap0"], arena["fmap1"], corr_sizes(case)[4], arena["workspace"])


def ondemand_lookup_call(D, ctx, arena, case, per_level):
    _, C, _, _, L, r = corr_sizes(case)
    D.corr_ondemand_lookup_device(ctx, arena["workspace"], C, L, r, arena["coords"], arena["out_per_level" if per_level else "out_fused"], per_level=per_level)


def _lookups_equal(arena, want, same, L, K, what):
    fused, per_level = _np(arena, "out_fused"), _np(arena, "out_per_level")
    assert same(fused, want), (what, "fused", _where(fused, want))
    assert same(per_level, per_level_form(want, L, K)), (what, "per level")


@pytest.mark.parametrize("case", CORR_CASES, ids=str)
def test_corr_pyramid_build_and_lookup_on_guarded_memory(ftk, case):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    f0, f1, c = corr_case(case)
    B, _, H, W, L, r = corr_sizes(case)
    levels, want = corr_want(case)
    _, offsets, dims = N.corr_pyramid_layout(B, H, W, L)
    inputs = dict(fmap0=f0, fmap1=f1, coords=c)
    for fill in FILLS:
        arena = make_arena(corr_specs(case), inputs, fill)
        ctx = _ctx(arena)
        corr_build_call(D, ctx, arena, case)
        host = _finish(arena, inputs)
        volume = _np(arena, "volume")
        for l, (off, (h, w)) in enumerate(zip(offsets, dims)):  # every level written, each exactly the restatement's
            got = volume[off:off + B * H * W * h * w].reshape(B * H * W, h, w)
            assert CR.same(got, levels[l]), (hex(fill), f"level {l}", _where(got, levels[l]))
        built = arena.payload_bytes("volume", host).copy()
        for per_level in (False, True):  # both lookups on the same guarded volume, which they only read
            corr_lookup_call(D, ctx, arena, case, per_level)
        _finish(arena, dict(inputs, volume=built))
        _lookups_equal(arena, want, CR.same, L, (2 * r + 1) ** 2, hex(fill))


@pytest.mark.parametrize("case", CORR_CASES, ids=str)
def test_corr_ondemand_prepare_and_lookup_on_guarded_memory(ftk, case):
    from feature_tracker_amd import device as D
    f0, f1, c = corr_case(case)
    _, _, _, _, L, r = corr_sizes(case)
    want = ondemand_want(case)
    inputs = dict(fmap0=f0, fmap1=f1, coords=c)
    prepared = []
    for fill in FILLS:
        arena = make_arena(ondemand_specs(case), inputs, fill)
        ctx = _ctx(arena)
        ondemand_prepare_call(D, ctx, arena, case)
        host = _finish(arena, inputs)
        prepared.append(arena.payload_bytes("workspace", host).copy())
        for per_level in (False, True):
            ondemand_lookup_call(D, ctx, arena, case, per_level)
        _finish(arena, dict(inputs, workspace=prepared[-1]))
        _lookups_equal(arena, want, CO.same, L, (2 * r + 1) ** 2, hex(fill))
    assert prepared[0].tobytes() == prepared[1].tobytes()  # every element of the workspace is written: the same bytes from zeros and from NaNs


# ---- flow_upsample_device ------------------------------------------------------------------------------------------------------------------
# (B, H, W, logit scale, mask_scale) from tests/test_flow_upsample_gpu.py's SHAPES (T = FTK_FLOW_UPSAMPLE_TILE = 32) and scales, and its
# hostile logits
UPSAMPLE_CASES = [(1, 1, 1, 1.0, 1.0), (1, 1, 9, 30.0, 0.25), (2, 3, 5, 1.0, 0.3), (1, 2, 31, 30.0, 0.3), (1, 2, 32, 1.0, 0.25), (1, 2, 33, 30.0, 0.3),
                  (2, 5, 67, 1.0, 0.3), "hostile"]


@functools.lru_cache(maxsize=None)
def upsample_case(case):
    if case == "hostile":
        flow, mask = hostile_inputs()
        scale = 1.0
    else:
        B, H, W, logit_scale, scale = case
        flow, mask = (t.numpy() for t in upsample_inputs(1000 * H + W, B, H, W, logit_scale))
    return _readonly(flow, mask, FU.upsample(flow, mask, scale)) + (scale,)


def upsample_specs(case):
    flow, mask, _, _ = upsample_case(case)
    B, _, H, W = flow.shape
    return [_spec("flow", flow), _spec("mask", mask), _spec("out", (B, 2, 8 * H, 8 * W))]


def upsample_call(D, ctx, arena, case):
    D.flow_upsample_device(ctx, arena["flow"], arena["mask"], arena["out"], upsample_case(case)[3])


@pytest.mark.parametrize("case", UPSAMPLE_CASES, ids=str)
def test_flow_upsample_on_guarded_memory(ftk, case):
    from feature_tracker_amd import device as D
    flow, mask, want, _ = upsample_case(case)
    inputs = dict(flow=flow, mask=mask)
    for fill in FILLS:
        arena = make_arena(upsample_specs(case), inputs, fill)
        upsample_call(D, _ctx(arena), arena, case)
        _finish(arena, inputs)
        got = _np(arena, "out")
        assert FU.same(got, want), (hex(fill), _where(got, want))


# ---- flow_warm_device ----------------------------------------------------------------------------------------------------------------------
# (kind, (H, W), B) of tests/test_flow_warm_gpu.py's case(): one pixel, one row, one column, below and above a tile of FTK_FLOW_WARM_TILE =
# 256, a row of one pixel more than a tile, and its largest shape at B 3 (an entry without a valid source, a zero entry)
WARM_CASES = [("sigma 2", (1, 1), 1), ("sigma 2", (1, 70), 1), ("sigma 40", (70, 1), 3), ("integers", (9, 17), 1), ("hostile", (1, 257), 1),
              ("hostile", (33, 65), 3)]
WARM_SPLITS = (1, 2, 5)  # one launch without a workspace; two ranges; more ranges than the small shapes have tiles of sources


def warm_splits(case):
    """WARM_SPLITS and the count the library itself would choose."""
    from feature_tracker_amd import _native as N
    kind, (H, W), B = case
    return sorted(set(WARM_SPLITS) | {N.flow_warm_splits(B, H, W)})


def warm_specs(case, splits):
    _, (H, W), B = case
    specs = [_spec("flow", (B, 2, H, W))]
    if splits > 1:
        specs.append(_spec("workspace", (splits * B * H * W,), "int64"))  # the declared size, with no added term
    return specs + [_spec("out", (B, 2, H, W))]


def warm_call(D, ctx, arena, case, splits):
    D.flow_warm_device(ctx, arena["flow"], arena["out"], splits, arena["workspace"] if splits > 1 else None)


@pytest.mark.parametrize("case", WARM_CASES, ids=str)
def test_flow_warm_on_guarded_memory(ftk, case):
    from feature_tracker_amd import device as D
    flow, want = warm_case(*case)
    for splits in warm_splits(case):
        for fill in FILLS:
            arena = make_arena(warm_specs(case, splits), dict(flow=flow), fill)
            warm_call(D, _ctx(arena), arena, case, splits)
            _finish(arena, dict(flow=flow))
            got = _np(arena, "out")
            assert FW.same(got, want), (splits, hex(fill), _where(got, want))


# ---- flow_track_points_device --------------------------------------------------------------------------------------------------------------
# the grids of tests/test_flow_points_cpu.py (one cell; 3 x 5; 2 x 33, a tile of 32 cells and one), the point counts around
# FTK_FLOW_POINTS_TILE = 64, both image sizes; point_set puts corners, points outside, +-inf and NaN points first
POINT_COUNTS = (1, 63, 64, 65)
POINT_FORMS = ("forward", "forward-backward", "forward-backward without fb_error2")


@functools.lru_cache(maxsize=None)
def points_case(grid, count, n):
    """(inputs by payload name, image size, mask_scale, the restatement's (cur_points, status, fb_error2) of the forward-backward form and
    of the forward form) for image size ``n`` of the grid."""
    B, H, W = grid
    image_size = image_sizes(H, W)[n]
    mask_scale = (1.0, 0.25, 0.3)[(n + count) % 3]
    flow, mask, flow_back, mask_back = fields(100 * H + W + count, B, H, W, (1.0, 30.0)[n])
    points = point_set(B, H, W, count, image_size, count)
    inputs = dict(flow=flow, mask=mask, points=points, flow_back=flow_back, mask_back=mask_back)
    _readonly(*inputs.values())
    both = FP.track(flow, mask, points, image_size, mask_scale, (flow_back, mask_back), 1.0)
    forward = FP.track(flow, mask, points, image_size, mask_scale)
    return inputs, image_size, mask_scale, both, forward


def points_specs(grid, count, form):
    B, H, W = grid
    specs = [_spec("flow", (B, 2, H, W)), _spec("mask", (B, 576, H, W)), _spec("points", (B, count, 2))]
    if form != "forward":
        specs += [_spec("flow_back", (B, 2, H, W)), _spec("mask_back", (B, 576, H, W))]
    specs += [_spec("cur_points", (B, count, 2)), _spec("status", (B, count), "uint8")]
    if form == "forward-backward":
        specs.append(_spec("fb_error2", (B, count)))
    return specs


def points_call(D, ctx, arena, form, image_size, mask_scale):
    back = form != "forward"
    D.flow_track_points_device(ctx, arena["flow"], arena["mask"], arena["points"], image_size[0], image_size[1], arena["cur_points"], arena["status"],
                               arena["fb_error2"] if form == "forward-backward" else None, mask_scale, arena["flow_back"] if back else None,
                               arena["mask_back"] if back else None, 1.0 if back else 0.0)


@pytest.mark.parametrize("count", POINT_COUNTS)
@pytest.mark.parametrize("grid", POINT_GRIDS, ids=str)
def test_flow_track_points_on_guarded_memory(ftk, grid, count):
    from feature_tracker_amd import device as D
    for n in range(2):
        inputs, image_size, mask_scale, both, forward = points_case(grid, count, n)
        for form in POINT_FORMS:
            want = forward if form == "forward" else both
            names = [s[0] for s in points_specs(grid, count, form)]
            given = {name: a for name, a in inputs.items() if name in names}
            for fill in FILLS:
                arena = make_arena(points_specs(grid, count, form), given, fill)
                points_call(D, _ctx(arena), arena, form, image_size, mask_scale)
                _finish(arena, given)
                what = (n, form, hex(fill))
                assert FP.same(_np(arena, "cur_points"), want[0]) and FP.same(_np(arena, "status"), want[1]), what
                if form == "forward-backward":
                    assert FP.same(_np(arena, "fb_error2"), want[2]), what
