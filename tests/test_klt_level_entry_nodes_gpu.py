"""The level entry of the pipelined Basic-inverse kernel (csrc/klt_basic_kernels.hip): node tables, node counts and lattice, at the places
where they can go wrong.

A patch row / column t has the coordinate x_t = float(t - h) + centre; its minus / plus taps sit at fl(x_t - 1) / fl(x_t + 1).  Where the
unit step crosses a power of two those differ bitwise from x_{t-1} / x_{t+1} and the axis gets an EXTRA node (build_nodes_pass), so the
node counts n_r / n_c, the index triples and the lattice size change from feature to feature.  The features below put the patch across the
coordinates 1, 2, 4, 8, 16, 32 and 64 on each axis alone and on both (with three levels the coarser levels see a quarter and a half of the
coordinate, so 64 -> 16 -> ... cross there too), and within one pixel of every border of the image, where nodes turn invalid.

Basic inverse through DeviceKlt.track, bitwise against the CPU oracle: positions as uint32, status, iteration counts; one and three levels;
a one-chunk patch (3x3), the headline patch (21x21), rows != columns (5x13: the two axes differ in length) and rows + columns > 64
(33x33: one node pass per axis); one, two and three waves per feature through FTK_KLT_WAVES.  The CPU tests say that every case runs the
pipelined kernel with the forced wave count and that the oracle really tracks features in it: two arrays of "not tracked" prove nothing."""
import functools

import numpy as np
import pytest

from tests import oracle_lib, scenes
from tests.test_klt_plan_cpu import BASIC, INVERSE, plan

WIDTH, HEIGHT, N = 96, 80, 64
TRACKED = 1
LEVELS = (1, 3)
PATCHES = {"3x3": (1, 1), "21x21": (10, 10), "5x13": (2, 6), "33x33": (16, 16)}  # rows x columns -> (half rows, half columns)
WAVES = (1, 2, 3)
BINADES = (1, 2, 4, 8, 16, 32, 64)


@functools.lru_cache(maxsize=None)
def pair(levels):
    from feature_tracker_amd import synth
    ref, cur = synth.make_image_pair(WIDTH, HEIGHT, (0.7, -0.5))  # a motion that a 3x3 patch on one level can still follow
    return tuple(synth.build_pyramid(ref, levels)), tuple(synth.build_pyramid(cur, levels))


@functools.lru_cache(maxsize=None)
def feature_positions():
    """(64, 2) float32 (u, v) = (column, row)."""
    mid_u, mid_v = 48.6, 40.3
    uv = []
    for b in BINADES:
        uv.append((b + 0.37, mid_v))   # the column axis straddles b from above: fl(x - 1) falls into the binade below
        uv.append((b - 0.29, mid_v))   # ... from below: fl(x + 1) rises into the binade above
        uv.append((mid_u, b + 0.37))   # the row axis
        uv.append((mid_u, b - 0.29))
        uv.append((b + 0.37, b - 0.29))  # both axes
    last_u, last_v = WIDTH - 1.0, HEIGHT - 1.0
    for u in (0.4, last_u - 0.3):      # within one pixel of the left / right border, and the four corners
        uv.append((u, mid_v))
        for v in (0.6, last_v - 0.5):
            uv.append((u, v))
    for v in (0.6, last_v - 0.5):      # top / bottom border
        uv.append((mid_u, v))
    uv += [(0.0, 0.0), (last_u, last_v)]  # on the border itself
    uv = np.float32(uv)
    assert len(uv) <= N
    fill = scenes.features(N - len(uv), WIDTH, HEIGHT, half=10, seed=4321)
    return np.ascontiguousarray(np.concatenate([uv, fill.astype(np.float32)], axis=0))


@functools.lru_cache(maxsize=None)
def oracle_result(levels, patch):
    hr, hc = PATCHES[patch]
    ref_levels, cur_levels = pair(levels)
    ok, uv, st, it = oracle_lib.klt_track_pyramid("basic", list(ref_levels), list(cur_levels), feature_positions(), method="inverse", half=hr, half_cols=hc,
                                                  max_points=N)
    for a in (uv, st, it):
        a.setflags(write=False)
    return ok, uv, st, it


CASES = [(lv, p) for lv in LEVELS for p in PATCHES]


def test_the_positions_cover_every_binade_and_border():
    uv = feature_positions().astype(np.float64)
    assert uv.shape == (N, 2) and (uv >= 0).all() and (uv[:, 0] <= WIDTH - 1).all() and (uv[:, 1] <= HEIGHT - 1).all()
    for axis in (0, 1):
        other = 1 - axis
        for b in BINADES:
            near = np.abs(uv[:, axis] - b) < 1.0  # the 3-pixel patch already has a row / column on each side of b
            assert (near & (uv[:, axis] > b)).any() and (near & (uv[:, axis] < b)).any(), (axis, b)
            assert (near & (np.abs(uv[:, other] - (48.6, 40.3)[other]) < 1e-3)).any(), ("alone", axis, b)
            assert (near & (np.abs(uv[:, other] - b) < 1.0)).any(), ("both", axis, b)
        last = (WIDTH, HEIGHT)[axis] - 1
        assert (uv[:, axis] < 1.0).any() and (uv[:, axis] > last - 1.0).any(), axis


@pytest.mark.parametrize("levels,patch", CASES, ids=[f"L{lv}-{p}" for lv, p in CASES])
def test_the_oracle_tracks_features_in_every_case(oracle, levels, patch):
    ok, uv, st, it = oracle_result(levels, patch)
    assert ok
    assert (st == TRACKED).sum() >= 1, f"no feature ends TRACKED: statuses {np.bincount(st, minlength=5)}"
    assert (it > 0).sum() >= N // 2, "most features must run iterations, not pass through"
    moved = (uv.view(np.uint32) != feature_positions().view(np.uint32)).any(axis=1)
    assert moved[st == TRACKED].all()


def test_every_case_plans_the_pipelined_kernel_with_the_forced_waves():
    cases = [dict(model=BASIC, method=INVERSE, half=PATCHES[p], n=N, max_extent=WIDTH, waves=w) for p in PATCHES for w in WAVES]
    for c, p in zip(cases, plan(cases)):
        assert p["form"] == "pipelined" and p["waves_per_feature"] == c["waves"] and p["solo"] == int(c["waves"] == 1), f"{c} -> {p}"


@pytest.fixture(scope="module")
def device_side():
    import torch
    from feature_tracker_amd import device as D
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        ctx = D.context_on_stream(stream, 0)
        pyramids = {lv: (D.upload_pyramid(pair(lv)[0], ctx, dev), D.upload_pyramid(pair(lv)[1], ctx, dev)) for lv in LEVELS}
        d_ref = torch.from_numpy(feature_positions()).to(dev)
    yield torch, D, dev, stream, ctx, pyramids, d_ref
    stream.synchronize()
    ctx.close()


GPU_CASES = [(lv, p, w) for lv, p in CASES for w in WAVES]


@pytest.mark.gpu
@pytest.mark.parametrize("levels,patch,waves", GPU_CASES, ids=[f"L{lv}-{p}-w{w}" for lv, p, w in GPU_CASES])
def test_level_entry_bits_equal_the_oracle(ftk, oracle, switch, device_side, levels, patch, waves):
    torch, D, dev, stream, ctx, pyramids, d_ref = device_side
    hr, hc = PATCHES[patch]
    ok, want_uv, want_st, want_it = oracle_result(levels, patch)
    assert ok
    switch("FTK_KLT_WAVES", waves)
    with torch.cuda.stream(stream):
        opt = ftk.OpticalFlowOptions()
        opt.kMethod, opt.kPatchRowHalfSize, opt.kPatchColHalfSize, opt.kMaxTrackPointsNumber = "inverse", hr, hc, N
        klt = D.DeviceKlt("basic", opt, pyramids[levels][0], pyramids[levels][1], ctx)
        d_out, d_st_out = torch.empty_like(d_ref), torch.empty(N, dtype=torch.uint8, device=dev)
        d_it = torch.zeros(N, dtype=torch.int32, device=dev)
        klt.track(d_ref, d_ref.clone(), torch.zeros(N, dtype=torch.uint8, device=dev), d_out, d_st_out, d_it)
        stream.synchronize()
    got_uv, got_st, got_it = d_out.cpu().numpy(), d_st_out.cpu().numpy(), d_it.cpu().numpy().astype(np.uint32)
    what = f"{levels} level(s), {patch}, {waves} wave(s)"
    assert np.array_equal(got_st, want_st), f"{what}: status differs at features {np.nonzero(got_st != want_st)[0][:10]}"
    assert np.array_equal(got_it, want_it), f"{what}: iteration counts differ at features {np.nonzero(got_it != want_it)[0][:10]}"
    diff = (got_uv.view(np.uint32) != want_uv.view(np.uint32)).any(axis=1)
    assert not diff.any(), f"{what}: {diff.sum()} of {N} positions differ in their bits, first features {np.nonzero(diff)[0][:10]}"
