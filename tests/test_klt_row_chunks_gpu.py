"""Row chunks of the pipelined Basic-inverse kernel (csrc/klt_basic_kernels.hip, pb_row_chunks): at 21x21 a chunk of the Gauss-Newton loop
is three whole patch rows (63 pixels and one idle lane) instead of 64 consecutive pixels of the row-major patch; 13x13, 11x11 and the
run-time geometry keep the linear chunks.  The sums must not notice: the terms meet the accumulator in the same row-major order, with one
exact zero behind every 63rd.

Basic inverse through DeviceKlt.track, bitwise against the CPU oracle (positions as uint32, status, iteration counts), on a 320x240 pair
with a constant block, 3 and 4 levels, at one, two and three waves per feature (FTK_KLT_WAVES).  The features are chosen so that a chunk
meets what could break it: patches across each image border on the finest and on the coarsest level (whole invalid rows, invalid
columns inside every chunk), a binade crossing inside the patch (an extra lattice node), a constant neighbourhood (every product +-0),
a start so far off that level 2 walks out of its window and restages it, and incoming statuses that pass through.  The CPU tests show from
the oracle's own results that these cases occur.  One case each at 13x13, 11x11 and 21x11 holds the linear instantiations and the
run-time geometry to the oracle, and one at 21x21 holds the throughput mode to its integer-exact anchor (tests/test_reduction_tree_gpu.py)."""
import functools

import numpy as np
import pytest

from tests import oracle_lib, scenes
from tests.test_klt_plan_cpu import BASIC, INVERSE, plan

WIDTH, HEIGHT = 320, 240
HALF = 10
LEVELS = (3, 4)
WAVES = (1, 2, 3)
FLAT = (200, 100, 270, 170)  # (col0, row0, col1, row1): constant in both images
TRACKED, OUTSIDE = 1, 3
OTHER_PATCHES = {"13x13": (6, 6), "11x11": (5, 5), "21x11": (10, 5)}  # linear chunks: two compile-time geometries and the run-time one

# the named features: (u, v) of the reference point, the start in the current image (None: the reference point), incoming status
NAMED = {
    "interior": ((150.3, 120.6), None, 0),
    "left_fine": ((3.4, 120.2), None, 0),          # within half a patch of a border on level 0
    "right_fine": ((WIDTH - 1 - 4.7, 90.6), None, 0),
    "top_fine": ((140.8, 2.9), None, 0),
    "bottom_fine": ((170.1, HEIGHT - 1 - 5.2), None, 0),
    "corner_fine": ((6.3, 5.1), None, 0),
    "left_coarse": ((30.3, 130.4), None, 0),       # clear of the border on level 0, across it from level 2 on (30.3 / 4 < 10)
    "right_coarse": ((WIDTH - 1 - 28.9, 110.2), None, 0),
    "top_coarse": ((120.7, 28.7), None, 0),
    "bottom_coarse": ((180.2, HEIGHT - 1 - 29.4), None, 0),
    "binade_u": ((64.37, 118.3), None, 0),         # columns 54 .. 74 straddle 64; 32.2, 16.1 and 8.05 on the levels above
    "binade_v": ((152.6, 127.71), None, 0),        # rows straddle 128 (and 64, 32, 16 above)
    "flat": ((235.0, 135.0), (235.0, 135.0), 0),   # the middle of the constant block: every product of level 0 is +-0
    "restage": ((100.4, 150.7), (100.4 + 3.3 - 16.0, 150.7 - 2.1 - 14.0), 0),  # starts 16 / 14 px off the true position: 4 / 3.5 px of level 2
    "tracked_in": ((210.6, 60.4), None, 1),        # incoming TRACKED: tracked again
    "failed_in_2": ((90.2, 70.9), None, 2),        # incoming failures: passed through untouched
    "failed_in_3": ((95.2, 75.9), None, 3),
    "failed_in_4": ((99.2, 79.9), None, 4),
}
N = 48


@functools.lru_cache(maxsize=None)
def pair(levels):
    from feature_tracker_amd import synth
    ref, cur = synth.make_image_pair(WIDTH, HEIGHT, (3.3, -2.1))
    c0, r0, c1, r1 = FLAT
    ref[r0:r1, c0:c1] = 128
    cur[r0:r1, c0:c1] = 128
    return tuple(synth.build_pyramid(ref, levels)), tuple(synth.build_pyramid(cur, levels))


@functools.lru_cache(maxsize=None)
def inputs(levels):
    """(ref uv, start uv, incoming status): the named features, then interior ones."""
    ref = [v[0] for v in NAMED.values()]
    start = [v[0] if v[1] is None else v[1] for v in NAMED.values()]
    status = [v[2] for v in NAMED.values()]
    fill = scenes.features(N - len(ref), WIDTH, HEIGHT, half=HALF, seed=777, border_fraction=0.0).astype(np.float32)
    ref_uv = np.ascontiguousarray(np.concatenate([np.float32(ref), fill]))
    start_uv = np.ascontiguousarray(np.concatenate([np.float32(start), fill]))
    st = np.concatenate([np.uint8(status), np.zeros(len(fill), np.uint8)])
    for a in (ref_uv, start_uv, st):
        a.setflags(write=False)
    return ref_uv, start_uv, st


def index(name):
    return list(NAMED).index(name)


@functools.lru_cache(maxsize=None)
def oracle_result(levels, half=(HALF, HALF)):
    ref_levels, cur_levels = pair(levels)
    ref_uv, start_uv, st = inputs(levels)
    ok, uv, st_out, it = oracle_lib.klt_track_pyramid("basic", list(ref_levels), list(cur_levels), ref_uv, start_uv, st, method="inverse", half=half[0],
                                                      half_cols=half[1], max_points=N)
    for a in (uv, st_out, it):
        a.setflags(write=False)
    return ok, uv, st_out, it


# ---- CPU: the chunk rule, the plans, and that the cases are what they are called ------------------------------------------------

def test_the_chunk_rule_takes_row_chunks_at_21x21_only():
    halves = [(10, 10), (6, 6), (5, 5), (10, 5)]
    cases = [dict(model=BASIC, method=INVERSE, half=h, n=N, max_extent=WIDTH, waves=w, tree=t) for h in halves for w in WAVES for t in (0, 1)]
    for c, p in zip(cases, plan(cases)):
        assert p["form"] == "pipelined" and p["waves_per_feature"] == c["waves"], f"{c} -> {p}"
        assert p["k_row_chunks"] == int(c["half"] == (10, 10)), f"{c} -> {p}"
        assert p["half"] == (c["half"][0] if c["half"][0] == c["half"][1] else 0), f"{c} -> {p}"
    # the rule itself (pb_row_chunks): whole rows per 64-lane chunk, taken only where the chunk count stays what it was
    def rule(rows, cols):
        per = 64 // cols
        return -(-rows // per) == -(-rows * cols // 64)
    assert rule(21, 21) and not rule(13, 13) and not rule(11, 11)
    assert 3 * 21 == 63 and 7 * 3 == 21  # seven chunks of 63 pixels and one idle lane: lane 63 never carries a pixel


@pytest.mark.parametrize("levels", LEVELS)
def test_the_cases_occur_in_the_oracle(oracle, levels):
    ok, uv, st, it = oracle_result(levels)
    assert ok
    ref_uv, start_uv, st_in = inputs(levels)
    ref_levels, cur_levels = pair(levels)
    print({name: (int(st[index(name)]), int(it[index(name)])) for name in NAMED})
    # pass-through: untouched position, status and no iteration; an incoming TRACKED is tracked again
    for name in ("failed_in_2", "failed_in_3", "failed_in_4"):
        k = index(name)
        assert st[k] == st_in[k] and it[k] == 0 and np.array_equal(uv[k].view(np.uint32), start_uv[k].view(np.uint32)), name
    assert it[index("tracked_in")] > 0 and st[index("tracked_in")] == TRACKED
    # interior and binade features track; each runs at least one iteration per level
    for name in ("interior", "binade_u", "binade_v"):
        assert st[index(name)] == TRACKED and it[index(name)] >= levels, name
    for axis, name in ((0, "binade_u"), (1, "binade_v")):  # a power of two strictly inside the patch's coordinates, on every level
        for lv in range(levels):
            x = float(ref_uv[index(name)][axis]) / (1 << lv)
            assert any(x - HALF < b < x + HALF for b in (8, 16, 32, 64, 128)), (name, lv)
    # borders: the patch of the reference point leaves the image on level 0 (fine) or only from a coarser level on (coarse), and
    # the feature still iterates, so chunks with invalid rows / columns are summed
    limit = (WIDTH - 1, HEIGHT - 1)
    for name in NAMED:
        if not name.endswith(("_fine", "_coarse")):
            continue
        k = index(name)
        out = [[not (0 <= float(ref_uv[k][a]) / (1 << lv) - HALF - 1 and float(ref_uv[k][a]) / (1 << lv) + HALF + 1 <= limit[a] // (1 << lv)) for a in (0, 1)]
               for lv in range(levels)]
        assert any(out[levels - 1]), name
        assert any(out[0]) == name.endswith("_fine"), name
        assert it[k] >= levels, f"{name}: {it[k]} iterations"
    # flat: the 25x25 neighbourhoods of the reference point and of the start are constant on level 0 in both images, so that every
    # product of the first level-0 iteration is +-0; whatever the oracle makes of a zero matrix is what the kernel has to make of it
    k = index("flat")
    u, v = int(ref_uv[k][0]), int(ref_uv[k][1])
    c0, r0, c1, r1 = FLAT
    assert c0 + 2 * HALF + 6 <= u < c1 - 2 * HALF - 6 and r0 + 2 * HALF + 6 <= v < r1 - 2 * HALF - 6
    for img in (ref_levels[0], cur_levels[0]):
        assert np.ptp(img[v - HALF - 2:v + HALF + 3, u - HALF - 2:u + HALF + 3]) == 0
    assert it[k] >= levels
    # restage: the pyramid walk done level by level (positions doubled from one level to the next, as TrackFeatures does): on
    # level 2 the feature's row moves by three whole pixels or more over several iterations; the window has two rows of margin on
    # either side of the footprint it was staged for (KltParams::cwin_margin), so it is staged again in mid-level
    k = index("restage")
    scale = np.float32(1 << (levels - 1))
    r, c = ref_uv[k:k + 1] / scale, start_uv[k:k + 1] / scale
    rows_moved, iterations = {}, {}
    for lv in range(levels - 1, -1, -1):
        ok1, end, st1, it1 = oracle_lib.klt_track_single("basic", ref_levels[lv], cur_levels[lv], r, c, None, method="inverse", half=HALF, max_points=1)
        assert ok1
        rows_moved[lv], iterations[lv] = int(np.floor(float(end[0][1])) - np.floor(float(c[0][1]))), int(it1[0])
        r, c = r * np.float32(2), end * np.float32(2)
    print(f"restage: rows moved {rows_moved}, iterations {iterations}")
    if levels == 3:  # (with four levels the 40x30 level pulls the start in by two rows, inside the margin, and level 2 has nothing left to walk)
        assert abs(rows_moved[2]) >= 3 and iterations[2] >= 3
    assert sum(iterations.values()) == it[k] and st[k] == TRACKED
    assert np.abs(uv[k].astype(np.float64) - ref_uv[k] - (3.3, -2.1)).max() < 0.5


@pytest.mark.parametrize("patch", list(OTHER_PATCHES))
def test_the_oracle_tracks_at_the_other_patches(oracle, patch):
    ok, uv, st, it = oracle_result(3, OTHER_PATCHES[patch])
    assert ok and (st == TRACKED).sum() >= N // 2 and (it > 0).sum() >= N - 3


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device_side():
    import torch
    from feature_tracker_amd import device as D
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        ctx = D.context_on_stream(stream, 0)
        pyramids = {lv: (D.upload_pyramid(pair(lv)[0], ctx, dev), D.upload_pyramid(pair(lv)[1], ctx, dev)) for lv in LEVELS}
        d_inputs = {lv: tuple(torch.from_numpy(a.copy()).to(dev) for a in inputs(lv)) for lv in LEVELS}
    yield torch, D, dev, stream, ctx, pyramids, d_inputs
    stream.synchronize()
    ctx.close()


def track_and_compare(ftk, switch, device_side, levels, half, waves, what):
    torch, D, dev, stream, ctx, pyramids, d_inputs = device_side
    d_ref, d_start, d_st = d_inputs[levels]
    ok, want_uv, want_st, want_it = oracle_result(levels, half)
    assert ok
    switch("FTK_KLT_WAVES", waves)
    with torch.cuda.stream(stream):
        opt = ftk.OpticalFlowOptions()
        opt.kMethod, opt.kPatchRowHalfSize, opt.kPatchColHalfSize, opt.kMaxTrackPointsNumber = "inverse", half[0], half[1], N
        klt = D.DeviceKlt("basic", opt, pyramids[levels][0], pyramids[levels][1], ctx)
        d_out, d_st_out = torch.empty_like(d_ref), torch.empty(N, dtype=torch.uint8, device=dev)
        d_it = torch.zeros(N, dtype=torch.int32, device=dev)
        klt.track(d_ref, d_start.clone(), d_st.clone(), d_out, d_st_out, d_it)
        stream.synchronize()
    got_uv, got_st, got_it = d_out.cpu().numpy(), d_st_out.cpu().numpy(), d_it.cpu().numpy().astype(np.uint32)
    assert np.array_equal(got_st, want_st), f"{what}: status differs at features {np.nonzero(got_st != want_st)[0][:10]}"
    assert np.array_equal(got_it, want_it), f"{what}: iteration counts differ at features {np.nonzero(got_it != want_it)[0][:10]}"
    diff = (got_uv.view(np.uint32) != want_uv.view(np.uint32)).any(axis=1)
    assert not diff.any(), f"{what}: {diff.sum()} of {N} positions differ in their bits, first features {np.nonzero(diff)[0][:10]}"


GPU_CASES = [(lv, w) for lv in LEVELS for w in WAVES]


@pytest.mark.gpu
@pytest.mark.parametrize("levels,waves", GPU_CASES, ids=[f"L{lv}-w{w}" for lv, w in GPU_CASES])
def test_row_chunk_bits_equal_the_oracle(ftk, oracle, switch, device_side, levels, waves):
    track_and_compare(ftk, switch, device_side, levels, (HALF, HALF), waves, f"21x21, {levels} levels, {waves} wave(s)")


@pytest.mark.gpu
@pytest.mark.parametrize("patch", list(OTHER_PATCHES))
def test_linear_chunk_bits_equal_the_oracle(ftk, oracle, switch, device_side, patch):
    track_and_compare(ftk, switch, device_side, 3, OTHER_PATCHES[patch], 2, f"{patch}, 3 levels, 2 waves")


@pytest.mark.gpu
@pytest.mark.parametrize("waves", (1, 2))
def test_tree_mode_with_row_chunks_is_bit_exact_on_an_integer_exact_scene(ftk, oracle, switch, waves):
    """The throughput mode at 21x21 against the anchor tests/test_reduction_tree_gpu.py holds it to: integer images, integer positions,
    one level and one iteration, every sum below 2^24 — every summation order gives the same floats, so a dropped or doubled term of a
    row chunk is a wrong bit."""
    from tests.test_reduction_tree_gpu import BASIC_SCENE as sc, assert_bits, oracle_track, track
    ref, cur = scenes.integer_scene(sc["width"], sc["height"], sc["lo"], sc["hi"], flat=sc["flat"])
    assert scenes.integer_sum_bound("basic", ref, cur, HALF, HALF) < 2 ** 24
    uv = scenes.integer_features(100, sc["width"], sc["height"], HALF, flat=sc["flat"])
    cpu = oracle_track(oracle_lib, "basic", "inverse", [ref], [cur], uv, HALF, HALF)
    assert not np.array_equal(cpu[1], uv)
    switch("FTK_KLT_WAVES", waves)
    ctx = ftk.Context()
    try:
        ctx.set_reduction("tree")
        assert_bits(track(ftk, ctx, "basic", "inverse", [ref], [cur], uv, HALF, HALF), cpu, f"tree 21x21 {waves} wave(s)")
    finally:
        ctx.close()
