"""Byte windows of the pipelined Basic-inverse kernel (csrc/klt_basic_kernels.hip; geometry and staging rule in csrc/ftk_device.h:
klt_byte_pitch, klt_byte_window_inside).  The kernel keeps its two image windows in LDS as plain bytes, rows a power-of-two pitch apart,
staged in 8-byte units, instead of 16-bit pixel pairs; a tap shifts its bytes out of aligned dwords.  Nothing of that may show in a result.

GPU part: Basic inverse through DeviceKlt.track, bitwise against the CPU oracle (positions as uint32, status, iteration counts), on small
images (160x120 and smaller) with 64 features: 21x21, 13x13, 11x11 (compile-time geometries), 21x11 and 15x9 (run-time geometry), 3 and 4
levels, one, two and three waves per feature (FTK_KLT_WAVES).  The features: a sweep along the right border one and a half pixels apart
(so that window origins fall on either side of both the pair rule `c_lo <= cols - wcols - 4` and the byte rule `c_lo <= cols - pitch`),
the other three borders, (0, 0), a constant block, pass-through statuses, a start far enough off that a level restages its current window.
Image widths that are odd and = 4 (mod 8), and an image narrower than the pitch (every window takes the element path on every level).
The throughput mode is held to the integer-exact anchor of tests/test_reduction_tree_gpu.py.

CPU part, through host/build/klt_plan_cli: pitches and prefetched units per thread, that the byte windows fit the regions carved for the
pairs, and the staging rule over every image size up to 40x40."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_lib, scenes
from tests.test_klt_plan_cpu import BASIC, EXE, INVERSE, plan

N = 64
TRACKED = 1
PATCHES = {"21x21": (10, 10), "13x13": (6, 6), "11x11": (5, 5), "21x11": (10, 5), "15x9": (7, 4)}  # (half rows, half cols); the last two: run-time geometry
LEVELS = (3, 4)
WAVES = (1, 2, 3)
# name -> (width, height, constant block (col0, row0, col1, row1))
SCENES = {
    "main": (160, 120, (96, 60, 150, 114)),
    "odd": (157, 119, (96, 60, 150, 114)),    # odd on every level: 157, 78 -> 39 -> 19
    "mod4": (156, 116, (96, 60, 150, 114)),   # 156 = 4 (mod 8), 78, 39
    "narrow": (30, 64, None),                 # narrower than the 32-byte pitch of every patch here, on every level
}


# ---- the geometry, restated (ftk_device.h klt_fill_geometry / klt_byte_pitch) ------------------------------------------------

def windows(half):
    """((ref rows, ref cols), (cur rows, cur cols)) of the pipelined kernel's windows."""
    pr, pc = 2 * half[0] + 1, 2 * half[1] + 1
    return (pr + 4, (pc + 4 + 3) & ~3), (pr + 3 + 4, (pc + 3 + 4 + 3) & ~3)


def pitch_of(cols):
    need = (cols + 1 + 7) & ~7  # cols + 1 bytes of a row are read; staged in 8-byte units
    pitch = 8
    while pitch < need:
        pitch *= 2
    return pitch


def room(rows, cols):
    return 2 * ((rows * cols + 3) & ~3)  # bytes of the region carved for rows x cols 16-bit pairs


# ---- scenes and features ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pair(scene, levels):
    from feature_tracker_amd import synth
    w, h, flat = SCENES[scene]
    ref, cur = synth.make_image_pair(w, h, (3.3, -2.1))
    if flat is not None:
        c0, r0, c1, r1 = flat
        ref[r0:r1, c0:c1] = 128
        cur[r0:r1, c0:c1] = 128
    return tuple(synth.build_pyramid(ref, levels)), tuple(synth.build_pyramid(cur, levels))


def named(scene):
    """(ref (u, v), start (None: the reference point), incoming status)."""
    w, h, flat = SCENES[scene]
    f = {
        "origin": ((0.0, 0.0), None, 0),
        "left": ((2.4, h * 0.5 + 0.2), None, 0),
        "top": ((w * 0.45 + 0.8, 1.9), None, 0),
        "bottom": ((w * 0.55 + 0.1, h - 1 - 3.2), None, 0),
        "corner": ((w - 1 - 1.3, h - 1 - 2.1), None, 0),
        "tracked_in": ((w * 0.4 + 0.6, h * 0.3 + 0.4), None, 1),
        "failed_in_2": ((w * 0.3 + 0.2, h * 0.35 + 0.9), None, 2),
        "failed_in_3": ((w * 0.35 + 0.2, h * 0.4 + 0.9), None, 3),
        "failed_in_4": ((w * 0.38 + 0.2, h * 0.45 + 0.9), None, 4),
        "restage": ((w * 0.42 + 0.4, h * 0.5 + 0.7), (w * 0.42 + 0.4 + 3.3 - 16.0, h * 0.5 + 0.7 - 2.1 - 14.0), 0),
    }
    if flat is not None:
        c0, r0, c1, r1 = flat
        f["flat"] = (((c0 + c1) // 2 + 0.0, (r0 + r1) // 2 + 0.0), None, 0)
    # the right border, floor(u) from w - 2 down over 1.5 * 26 = 39 columns: more than the widest pitch here (32) + 4
    for k in range(26):
        f[f"right_{k}"] = ((w - 1.7 - 1.5 * k, 12.3 + (k * 17) % max(h - 24, 1)), None, 0)
    return f


@functools.lru_cache(maxsize=None)
def inputs(scene):
    w, h, _ = SCENES[scene]
    f = named(scene)
    ref = [v[0] for v in f.values()]
    start = [v[0] if v[1] is None else v[1] for v in f.values()]
    status = [v[2] for v in f.values()]
    rs = np.random.RandomState(4242)
    fill = np.stack([6.0 + rs.random_sample(N - len(ref)) * (w - 12.0), 6.0 + rs.random_sample(N - len(ref)) * (h - 12.0)], axis=1).astype(np.float32)
    ref_uv = np.ascontiguousarray(np.concatenate([np.float32(ref), fill]))
    start_uv = np.ascontiguousarray(np.concatenate([np.float32(start), fill]))
    st = np.concatenate([np.uint8(status), np.zeros(len(fill), np.uint8)])
    for a in (ref_uv, start_uv, st):
        a.setflags(write=False)
    return ref_uv, start_uv, st


def index(scene, name):
    return list(named(scene)).index(name)


@functools.lru_cache(maxsize=None)
def oracle_result(scene, levels, half):
    ref_levels, cur_levels = pair(scene, levels)
    ref_uv, start_uv, st = inputs(scene)
    ok, uv, st_out, it = oracle_lib.klt_track_pyramid("basic", list(ref_levels), list(cur_levels), ref_uv, start_uv, st, method="inverse", half=half[0],
                                                      half_cols=half[1], max_points=N)
    for a in (uv, st_out, it):
        a.setflags(write=False)
    return ok, uv, st_out, it


# ---- CPU: the plan's pitches and units, the fit, the staging rule, and that the cases are what they are called -----------------------

def test_pitches_and_units_per_thread():
    cases = [dict(model=BASIC, method=INVERSE, half=h, n=N, max_extent=160, waves=w, tree=t) for h in PATCHES.values() for w in WAVES for t in (0, 1)]
    for c, p in zip(cases, plan(cases)):
        what = f"{c} -> {p}"
        (rr, rc), (cr, cc) = windows(c["half"])
        assert p["form"] == "pipelined" and p["waves_per_feature"] == c["waves"], what
        assert (p["pb_rwin_rows"], p["pb_rwin_cols"], p["cwin_rows"], p["cwin_cols"]) == (rr, rc, cr, cc), what
        assert (p["pb_rwin_pitch"], p["pb_cwin_pitch"]) == (pitch_of(rc), pitch_of(cc)) and p["byte_windows_ok"] == 1, what
        if p["half"] == 0:  # run-time geometry: the slot counts of the pair staging, larger windows are staged after the lattice
            assert (p["k_ref_units"], p["k_cur_units"]) == (3, 4), what
        else:               # compile-time: what the windows need on the form's fewest threads (one wave solo, two otherwise)
            threads = 64 if c["waves"] == 1 else 128
            assert p["k_ref_units"] == -(-rr * pitch_of(rc) // 8 // threads) and p["k_cur_units"] == -(-cr * pitch_of(cc) // 8 // threads), what
    # the headline: 21x21 on two waves, a 32-byte pitch, one 8-byte unit per thread and window
    p = plan([dict(model=BASIC, method=INVERSE, half=(10, 10), n=2000)])[0]
    assert (p["waves_per_feature"], p["pb_rwin_pitch"], p["pb_cwin_pitch"], p["k_ref_units"], p["k_cur_units"]) == (2, 32, 32, 1, 1), p
    assert (p["pb_rwin_rows"] * 4, p["cwin_rows"] * 4) == (100, 112) and max(p["pb_rwin_rows"], p["cwin_rows"]) * 4 <= 128


def test_byte_windows_fit_the_carved_regions():
    halves = [(a, b) for a in range(0, 33) for b in range(0, 33)]
    cases = [dict(model=BASIC, method=INVERSE, half=h, n=300, max_extent=160) for h in halves]
    seen = 0
    for c, p in zip(cases, plan(cases)):
        if p["form"] != "pipelined":
            continue
        seen += 1
        what = f"{c} -> {p}"
        for rows, cols, pitch in ((p["pb_rwin_rows"], p["pb_rwin_cols"], p["pb_rwin_pitch"]), (p["cwin_rows"], p["cwin_cols"], p["pb_cwin_pitch"])):
            assert pitch == pitch_of(cols) and pitch & (pitch - 1) == 0 and pitch % 8 == 0, what
            assert pitch >= cols + 1, what                     # a tap of the last element reads one byte to the right
            assert rows * pitch <= room(rows, cols), what      # inside the region pb_lds_bytes reserves
        assert p["byte_windows_ok"] == 1, what
    assert seen >= 32 * 32


def test_the_staging_rule_keeps_every_unit_inside_its_image_row():
    """The rule's answers come from klt_byte_window_inside and the units' places from klt_byte_unit_offset, the two functions the kernel's
    staging uses (`klt_plan_cli inside` / `units`); what is computed here is only origin + unit offset + byte 0 .. 7."""
    lo, margin = -4, 4
    sizes = [(r, c) for r in range(1, 41) for c in range(1, 41)]
    for wrows, pitch in ((25, 32), (5, 16), (13, 16), (3, 8)):  # 21x21's reference window; smaller ones, so that many origins pass at these sizes
        text = "".join(f"{r} {c} {wrows} {pitch} {lo} {margin}\n" for r, c in sizes)
        out = subprocess.run([EXE, "inside"], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert len(lines) == len(sizes)
        out = subprocess.run([EXE, "units"], input="".join(f"{c} {wrows} {pitch}\n" for c in range(1, 41)), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        units = {c: np.array(line.split(), np.int64) for c, line in zip(range(1, 41), out.stdout.splitlines())}
        assert all(len(u) == wrows * pitch // 8 for u in units.values()) and len(units) == 40
        passed = 0
        for (rows, cols), line in zip(sizes, lines):
            yes = (np.frombuffer(line.encode(), np.uint8) == ord("1")).reshape(rows + margin - lo, cols + margin - lo)
            r_lo, c_lo = np.meshgrid(np.arange(lo, rows + margin), np.arange(lo, cols + margin), indexing="ij")
            if yes.any():
                # every byte every unit touches, for every origin the rule accepts: [origins, units, 8]
                first = (r_lo[yes] * cols + c_lo[yes])[:, None] + units[cols][None, :]
                touched = first[:, :, None] + np.arange(8)[None, None, :]
                assert touched.min() >= 0 and touched.max() < rows * cols, (rows, cols, wrows, pitch)
                # ... lies in the image row of its window row: unit idx belongs to window row idx // (pitch / 8)
                want_row = r_lo[yes][:, None] + (np.arange(len(units[cols])) // (pitch // 8))[None, :]
                assert np.array_equal(touched // cols, np.broadcast_to(want_row[:, :, None], touched.shape)), (rows, cols, wrows, pitch)
                # ... and the units of a window row are its bytes c_lo .. c_lo + pitch - 1, each once, in LDS order
                cols_touched = (touched % cols).reshape(len(first), wrows, pitch)
                assert np.array_equal(cols_touched, np.broadcast_to((c_lo[yes][:, None] + np.arange(pitch)[None, :])[:, None, :], cols_touched.shape))
            clear = (r_lo >= 0) & (r_lo + wrows <= rows) & (c_lo >= 0) & (c_lo + pitch <= cols)  # `pitch` columns clear of the right border
            assert not (clear & ~yes).any(), (rows, cols, wrows, pitch)
            passed += int(yes.sum())
        assert passed > 0 or pitch > 40 - 1, (wrows, pitch)
        if (wrows, pitch) != (25, 32):
            assert passed > 1000


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("patch", list(PATCHES))
def test_the_cases_occur_in_the_oracle(oracle, patch, levels):
    half = PATCHES[patch]
    ok, uv, st, it = oracle_result("main", levels, half)
    assert ok
    ref_uv, start_uv, st_in = inputs("main")
    ref_levels, cur_levels = pair("main", levels)
    w, h, flat = SCENES["main"]
    print({name: (int(st[index("main", name)]), int(it[index("main", name)])) for name in named("main")})
    for name in ("failed_in_2", "failed_in_3", "failed_in_4"):
        k = index("main", name)
        assert st[k] == st_in[k] and it[k] == 0 and np.array_equal(uv[k].view(np.uint32), start_uv[k].view(np.uint32)), name
    assert it[index("main", "tracked_in")] > 0
    assert it[index("main", "origin")] > 0 and it[index("main", "flat")] > 0
    # flat: the footprint of the reference point is constant on level 0 in both images
    u, v = int(ref_uv[index("main", "flat")][0]), int(ref_uv[index("main", "flat")][1])
    for img in (ref_levels[0], cur_levels[0]):
        assert np.ptp(img[v - half[0] - 2:v + half[0] + 3, u - half[1] - 2:u + half[1] + 3]) == 0
    # the right sweep: on level 0 the current window's origin (floor(u) - half - 1 - margin 2) falls before, between and behind the two
    # rules for every patch: inside for both, inside for the pairs only (where the pitch is wider than cols + 4), outside for both
    for hh in PATCHES.values():
        (_, _), (_, ccols) = windows(hh)
        pitch = pitch_of(ccols)
        c_lo = [int(np.floor(ref_uv[index("main", f"right_{k}")][0])) - hh[1] - 3 for k in range(26)]
        old = [c <= w - ccols - 4 for c in c_lo]
        new = [c <= w - pitch for c in c_lo]
        assert any(new) and not all(old) and all(o or not n for o, n in zip(old, new)), hh
        if pitch > ccols + 4:
            assert sum(o and not n for o, n in zip(old, new)) >= 2, hh
    swept = [index("main", f"right_{k}") for k in range(26)]
    assert (it[swept] >= levels).sum() >= 20
    # restage: walked level by level, the feature moves three whole rows or more on one level over several iterations — beyond the two
    # rows of margin around the footprint its current window was staged for
    k = index("main", "restage")
    scale = np.float32(1 << (levels - 1))
    r, c = ref_uv[k:k + 1] / scale, start_uv[k:k + 1] / scale
    moved, iterations = {}, {}
    for lv in range(levels - 1, -1, -1):
        ok1, end, st1, it1 = oracle_lib.klt_track_single("basic", ref_levels[lv], cur_levels[lv], r, c, None, method="inverse", half=half[0], half_cols=half[1], max_points=1)
        assert ok1
        moved[lv] = max(abs(int(np.floor(float(end[0][1])) - np.floor(float(c[0][1])))), abs(int(np.floor(float(end[0][0])) - np.floor(float(c[0][0])))) - 1)
        iterations[lv] = int(it1[0])
        r, c = r * np.float32(2), end * np.float32(2)
    print(f"restage: moved {moved}, iterations {iterations}")
    if levels == 3:
        assert any(moved[lv] >= 3 and iterations[lv] >= 3 for lv in moved)
    assert sum(iterations.values()) == it[k]


def test_the_narrow_image_is_narrower_than_every_pitch():
    w = SCENES["narrow"][0]
    for hh in PATCHES.values():
        (_, rc), (_, cc) = windows(hh)
        assert w < pitch_of(rc) and w < pitch_of(cc)  # no origin passes the staging rule on any level
    assert SCENES["odd"][0] % 2 == 1 and SCENES["mod4"][0] % 8 == 4


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device_side():
    import torch
    from feature_tracker_amd import device as D
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        ctx = D.context_on_stream(stream, 0)
    cache = {}

    def get(scene, levels):
        if (scene, levels) not in cache:
            with torch.cuda.stream(stream):
                ref_levels, cur_levels = pair(scene, levels)
                cache[(scene, levels)] = (D.upload_pyramid(ref_levels, ctx, dev), D.upload_pyramid(cur_levels, ctx, dev),
                                          tuple(torch.from_numpy(a.copy()).to(dev) for a in inputs(scene)))
        return cache[(scene, levels)]

    yield torch, D, dev, stream, ctx, get
    stream.synchronize()
    ctx.close()


def track_and_compare(ftk, switch, device_side, scene, levels, half, waves):
    torch, D, dev, stream, ctx, get = device_side
    what = f"{scene} {2 * half[0] + 1}x{2 * half[1] + 1}, {levels} levels, {waves} wave(s)"
    ok, want_uv, want_st, want_it = oracle_result(scene, levels, half)
    assert ok
    d_ref_pyr, d_cur_pyr, (d_ref, d_start, d_st) = get(scene, levels)
    switch("FTK_KLT_WAVES", waves)
    with torch.cuda.stream(stream):
        opt = ftk.OpticalFlowOptions()
        opt.kMethod, opt.kPatchRowHalfSize, opt.kPatchColHalfSize, opt.kMaxTrackPointsNumber = "inverse", half[0], half[1], N
        klt = D.DeviceKlt("basic", opt, d_ref_pyr, d_cur_pyr, ctx)
        d_out, d_st_out = torch.empty_like(d_ref), torch.empty(N, dtype=torch.uint8, device=dev)
        d_it = torch.zeros(N, dtype=torch.int32, device=dev)
        klt.track(d_ref, d_start.clone(), d_st.clone(), d_out, d_st_out, d_it)
        stream.synchronize()
    got_uv, got_st, got_it = d_out.cpu().numpy(), d_st_out.cpu().numpy(), d_it.cpu().numpy().astype(np.uint32)
    names = list(named(scene))
    label = lambda ks: [names[k] if k < len(names) else int(k) for k in ks[:10]]
    assert np.array_equal(got_st, want_st), f"{what}: status differs at {label(np.nonzero(got_st != want_st)[0])}"
    assert np.array_equal(got_it, want_it), f"{what}: iteration counts differ at {label(np.nonzero(got_it != want_it)[0])}"
    diff = (got_uv.view(np.uint32) != want_uv.view(np.uint32)).any(axis=1)
    assert not diff.any(), f"{what}: {diff.sum()} of {N} positions differ in their bits, first {label(np.nonzero(diff)[0])}"


MAIN_CASES = [(p, lv, w) for p in PATCHES for lv in LEVELS for w in WAVES]


@pytest.mark.gpu
@pytest.mark.parametrize("patch,levels,waves", MAIN_CASES, ids=[f"{p}-L{lv}-w{w}" for p, lv, w in MAIN_CASES])
def test_byte_window_bits_equal_the_oracle(ftk, oracle, switch, device_side, patch, levels, waves):
    track_and_compare(ftk, switch, device_side, "main", levels, PATCHES[patch], waves)


WIDTH_CASES = [(s, p, lv) for s in ("odd", "mod4") for p in ("21x21", "13x13", "15x9") for lv in LEVELS]


@pytest.mark.gpu
@pytest.mark.parametrize("scene,patch,levels", WIDTH_CASES, ids=[f"{s}-{p}-L{lv}" for s, p, lv in WIDTH_CASES])
def test_odd_and_half_unit_widths_equal_the_oracle(ftk, oracle, switch, device_side, scene, patch, levels):
    track_and_compare(ftk, switch, device_side, scene, levels, PATCHES[patch], 2)


NARROW_CASES = [(p, lv, w) for p in ("21x21", "13x13", "11x11", "15x9") for lv in LEVELS for w in (1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("patch,levels,waves", NARROW_CASES, ids=[f"{p}-L{lv}-w{w}" for p, lv, w in NARROW_CASES])
def test_an_image_narrower_than_the_pitch_equals_the_oracle(ftk, oracle, switch, device_side, patch, levels, waves):
    track_and_compare(ftk, switch, device_side, "narrow", levels, PATCHES[patch], waves)


@pytest.mark.gpu
@pytest.mark.parametrize("half,waves", [(10, 1), (10, 2), (10, 3), (6, 2), (7, 2)])
def test_tree_mode_is_bit_exact_on_an_integer_exact_scene(ftk, oracle, switch, half, waves):
    """The throughput mode against the exact-sum yardstick of tests/test_reduction_tree_gpu.py: integer images, integer positions, one
    level and one iteration, every sum below 2^24, so every summation order gives the same floats and a wrong window byte is a wrong bit."""
    from tests.test_reduction_tree_gpu import BASIC_SCENE as sc, assert_bits, oracle_track, track
    ref, cur = scenes.integer_scene(sc["width"], sc["height"], sc["lo"], sc["hi"], flat=sc["flat"])
    assert scenes.integer_sum_bound("basic", ref, cur, half, half) < 2 ** 24
    uv = scenes.integer_features(100, sc["width"], sc["height"], half, flat=sc["flat"])
    cpu = oracle_track(oracle_lib, "basic", "inverse", [ref], [cur], uv, half, half)
    assert not np.array_equal(cpu[1], uv)
    switch("FTK_KLT_WAVES", waves)
    ctx = ftk.Context()
    try:
        ctx.set_reduction("tree")
        assert_bits(track(ftk, ctx, "basic", "inverse", [ref], [cur], uv, half, half), cpu, f"tree {2 * half + 1}x{2 * half + 1} {waves} wave(s)")
    finally:
        ctx.close()
