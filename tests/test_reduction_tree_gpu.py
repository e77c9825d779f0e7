"""The throughput reduction mode (ftk_set_reduction_mode(ctx, FTK_REDUCTION_TREE)) against references that do not lean on the exact
mode being close:

1. Integer-exact anchor: on low-contrast integer images, features at integer positions, one level and one iteration, every
   normal-equation term is an integer and every partial sum stays below 2^24, so every summation order gives the same float sums.
   The tree mode must then equal the oracle BIT FOR BIT: a dropped, duplicated or misplaced term is a wrong bit.  Each test asserts
   its premise (the sum bound) first.
2. Rounding regime: off those scenes, against the wide-sum oracle (oracle_lib.wide(): the same f32 products, sums in double): per
   feature e = |uv - uv_wide|_inf; max e_tree <= 4 max e_exact + 2 ulp and median e_tree <= median e_exact + ulp
   (scenes.rounding_regime; tests/test_reduction_oracle_cpu.py shows that a lost lane partial fails it by a wide margin).
3. What stays exact under the tree mode (ftk.h): affine inverse / direct, and the large-patch (spill) form.

The launch shapes are pinned with the library's switches so that every tree instantiation runs: the pipelined Basic-inverse kernel
(solo / multi-wave x compile-time halves 5, 6, 10 and the run-time geometry), the generic kernel's SOLO and multi-wave forms of
every variant, the chunked one-wave LSSD-fast level, and direct_track_kernel<true>."""
import numpy as np
import pytest

from tests import oracle_lib, scenes

pytestmark = pytest.mark.gpu

CLASSES = {"basic": "OpticalFlowBasicKlt", "affine": "OpticalFlowAffineKlt", "lssd": "OpticalFlowLssdKlt"}
VARIANTS = [(m, k, False) for m in ("basic", "affine", "lssd") for k in ("inverse", "direct", "fast")] + [("lssd", "fast", True)]

# (id, half rows, half cols, FTK_KLT_WAVES, FTK_KLT_GROUP, FTK_KLT_TAIL_CLASS, features); None leaves the library's choice
SHAPES = [
    ("h5-w1g1", 5, 5, 1, 1, "0", 100),
    ("h5-w2", 5, 5, 2, None, "1", 100),
    ("h6-w1g4", 6, 6, 1, 4, None, 100),
    ("h6-w4", 6, 6, 4, None, "0", 100),
    ("h10-w1g1", 10, 10, 1, 1, "1", 100),
    ("h10-w2", 10, 10, 2, None, None, 100),
    ("h3x7-w1g4", 3, 7, 1, 4, None, 100),
    ("h3x7-w4", 3, 7, 4, None, "1", 100),
    ("h15-w2", 15, 15, 2, None, "0", 100),
    ("h33", 33, 33, None, None, None, 40),
    ("h6-n1", 6, 6, None, None, None, 1),
    ("h6-n5000-w2", 6, 6, 2, None, "1", 5000),
    ("h6-n5000-w1", 6, 6, 1, 1, None, 5000),
]
SHAPE_IDS = [s[0] for s in SHAPES]

BASIC_SCENE = dict(width=320, height=240, lo=100, hi=160, flat=(200, 150, 300, 225))
AFFINE_SCENE = dict(width=32, height=24, lo=126, hi=130, flat=(20, 15, 30, 22))


@pytest.fixture(scope="module")
def contexts(ftk):
    tree, exact = ftk.Context(), ftk.Context()
    tree.set_reduction("tree")
    yield tree, exact
    tree.close()
    exact.close()


def pin(switch, shape):
    _, _, _, waves, group, tail, _ = shape
    switch("FTK_KLT_WAVES", waves)
    switch("FTK_KLT_GROUP", group)
    switch("FTK_KLT_TAIL_CLASS", tail)


def track(ftk, ctx, model, method, ref_levels, cur_levels, uv, half, half_cols=None, luminance=False, cur_uv=None, max_iteration=1):
    klt = getattr(ftk, CLASSES[model])(ctx)
    o = klt.options()
    o.kMethod, o.kPatchRowHalfSize, o.kPatchColHalfSize = method, half, half if half_cols is None else half_cols
    o.kMaxTrackPointsNumber, o.kMaxIteration = 100000, max_iteration
    if model == "lssd":
        klt.consider_patch_luminance = luminance
    rp, cp = ftk.ImagePyramid.from_host_levels(list(ref_levels), ctx), ftk.ImagePyramid.from_host_levels(list(cur_levels), ctx)
    ok, c, s = klt.TrackFeatures(rp, cp, uv, cur_uv, None)
    return ok, c, s, klt.last_iterations


def oracle_track(lib, model, method, ref_levels, cur_levels, uv, half, half_cols=None, luminance=False, cur_uv=None, max_iteration=1):
    return lib.klt_track_pyramid(model, list(ref_levels), list(cur_levels), uv, cur_uv, None, consider_luminance=luminance, method=method, half=half,
                                 half_cols=half_cols, max_points=100000, max_iteration=max_iteration)


def assert_bits(gpu, cpu, what):
    ok_g, uv_g, st_g, it_g = gpu
    ok_c, uv_c, st_c, it_c = cpu
    assert ok_g == ok_c, what
    assert np.array_equal(st_g, st_c), f"{what}: status differs at {np.nonzero(st_g != st_c)[0][:10]}"
    diff = (uv_g.view(np.uint32) != uv_c.view(np.uint32)).any(axis=1)
    assert not diff.any(), f"{what}: {diff.sum()} of {len(diff)} positions differ, first {np.nonzero(diff)[0][:5]}"
    assert np.array_equal(it_g, it_c), f"{what}: iteration counts differ"


# ---- 1. integer-exact anchor -------------------------------------------------------------------------------------------------

ANCHOR = [(m, k, s) for s in SHAPES for (m, k) in (("basic", "inverse"), ("basic", "direct"), ("basic", "fast"))] + \
         [(m, k, s) for s in SHAPES if max(s[1], s[2]) <= 7 for (m, k) in (("affine", "fast"), ("affine", "inverse"), ("affine", "direct"))]


@pytest.mark.parametrize("model,method,shape", ANCHOR, ids=[f"{m}-{k}-{s[0]}" for m, k, s in ANCHOR])
def test_tree_mode_is_bit_exact_on_integer_exact_scenes(ftk, contexts, switch, model, method, shape):
    sc = AFFINE_SCENE if model == "affine" else BASIC_SCENE
    _, hr, hc, _, _, _, n = shape
    ref, cur = scenes.integer_scene(sc["width"], sc["height"], sc["lo"], sc["hi"], flat=sc["flat"])
    bound = scenes.integer_sum_bound(model, ref, cur, hr, hc)
    assert bound < 2 ** 24, f"premise: sum |term| may reach {bound} >= 2^24 - the scene is wrong, not the kernel"
    uv = scenes.integer_features(n, sc["width"], sc["height"], max(hr, hc), flat=sc["flat"])
    pin(switch, shape)
    cpu = oracle_track(oracle_lib, model, method, [ref], [cur], uv, hr, hc)
    assert not np.array_equal(cpu[1], uv) or n == 1, "the scene must move the features"
    calls = 4 if n >= 1024 else 2  # from the third call of >= 1 024 features on: the longest-first launch order (sort block)
    for call in range(calls):
        gpu = track(ftk, contexts[0], model, method, [ref], [cur], uv, hr, hc)
        assert_bits(gpu, cpu, f"tree {model}/{method} {shape[0]} call {call}")


# ---- 2. rounding regime against the wide-sum oracle ---------------------------------------------------------------------------

def regime(ftk, contexts, model, method, luminance, ref_levels, cur_levels, uv, hr, hc, what, calls=2):
    """GPU exact == oracle (bits); GPU tree vs the wide oracle: statuses and the criterion; repeated tree calls are bit-identical."""
    tree_ctx, exact_ctx = contexts
    cpu = oracle_track(oracle_lib, model, method, ref_levels, cur_levels, uv, hr, hc, luminance)
    wide = oracle_track(oracle_lib.wide(), model, method, ref_levels, cur_levels, uv, hr, hc, luminance)
    assert_bits(track(ftk, exact_ctx, model, method, ref_levels, cur_levels, uv, hr, hc, luminance), cpu, f"exact {what}")
    first = track(ftk, tree_ctx, model, method, ref_levels, cur_levels, uv, hr, hc, luminance)
    for call in range(1, calls):  # same call, same launch shape: bit-identical
        again = track(ftk, tree_ctx, model, method, ref_levels, cur_levels, uv, hr, hc, luminance)
        assert np.array_equal(again[1].view(np.uint32), first[1].view(np.uint32)) and np.array_equal(again[2], first[2]), f"tree {what}: call {call} differs"
    ok, uv_tree, st_tree, _ = first
    assert ok == wide[0]
    uv_wide, st_wide = wide[1].astype(np.float64), wide[2]
    # statuses: a feature whose wide step lies within 1e-3 (relative) of a threshold may flip; so may one whose status the f32
    # chain's own rounding flips (exact != wide), or whose position it moves by more than 0.1 px (near-singular normal equations;
    # LSSD's step also holds the angle, which the positions do not show), or whose one step leaves the patch's footprint (the real
    # pair has LSSD features that jump 90 px, and a 1e-4 px nudge of the input sends them outside).  Counted and printed: up to
    # 5.5 % of the real pair's LSSD features, fewer elsewhere.
    rows, cols = ref_levels[0].shape
    step = uv_wide - uv.astype(np.float64)
    sq = (step ** 2).sum(axis=1)
    near = np.abs(sq - 4e-2) <= 1e-3 * 4e-2
    for k, lim in ((0, cols - 1), (1, rows - 1)):
        near |= np.abs(uv_wide[:, k]) <= 1e-3 * lim
        near |= np.abs(uv_wide[:, k] - lim) <= 1e-3 * lim
    near |= cpu[2] != st_wide
    near |= ~(np.abs(cpu[1].astype(np.float64) - uv_wide) <= 0.1).all(axis=1)
    near |= ~(np.abs(step) <= max(hr, hc) + 1).all(axis=1)
    bad = (st_tree != st_wide) & ~near
    assert not bad.any(), f"tree {what}: status differs from the wide oracle at {np.nonzero(bad)[0][:10]}"
    assert near.sum() <= 0.08 * len(uv) + 1, f"tree {what}: {near.sum()} features at a threshold"
    ok, msg, ratio = scenes.rounding_regime(uv_tree, cpu[1], wide[1], f"tree {what}")
    print(f"{msg}; {near.sum()} at a threshold; error / bound {ratio:.3f}")
    assert ok, msg


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("model,method,luminance", VARIANTS, ids=[f"{m}-{k}{'-lum' if l else ''}" for m, k, l in VARIANTS])
def test_tree_mode_rounds_no_worse_than_the_exact_chain(ftk, contexts, switch, model, method, luminance, shape):
    _, hr, hc, _, _, _, n = shape
    ref_levels, cur_levels = scenes.scene(320, 240, 1, "easy", "similarity" if model != "basic" else "translation")
    uv = scenes.features(n, 320, 240, half=min(max(hr, hc), 20))
    pin(switch, shape)
    regime(ftk, contexts, model, method, luminance, ref_levels, cur_levels, uv, hr, hc, f"{model}/{method}{' lum' if luminance else ''} {shape[0]}")


@pytest.mark.parametrize("chunked", ["1", "0"])
@pytest.mark.parametrize("model,method,luminance", VARIANTS, ids=[f"{m}-{k}{'-lum' if l else ''}" for m, k, l in VARIANTS])
def test_tree_mode_on_the_real_pair(ftk, contexts, switch, model, method, luminance, chunked):
    """The reference's example pair, level 0, 1 500 features (long-tail class and launch order from 1 024 on); one wave per
    feature for LSSD fast, with the chunked level (part[9] + butterfly) and without it."""
    from tests.test_klt_gpu import _real_pair
    ref_levels, cur_levels = _real_pair()
    rows, cols = ref_levels[0].shape
    rs = np.random.RandomState(5)
    uv = np.stack([rs.uniform(30, cols - 30, 1500), rs.uniform(30, rows - 30, 1500)], axis=1).astype(np.float32)
    switch("FTK_KLT_TAIL_CLASS", "1")
    if model == "lssd" and method == "fast":
        switch("FTK_KLT_WAVES", "1")
        switch("FTK_LSSD_CHUNKED", chunked)
    elif chunked == "0":
        switch("FTK_KLT_WAVES", "2")
    regime(ftk, contexts, model, method, luminance, ref_levels[:1], cur_levels[:1], uv, 6, 6, f"real {model}/{method}{' lum' if luminance else ''} chunked={chunked}",
           calls=4)


# ---- direct method: direct_track_kernel<true> -------------------------------------------------------------------------------

def _direct_regime(tree, exact, wide, what):
    pose = lambda r: np.concatenate([np.asarray(r[0], np.float32), np.asarray(r[1], np.float32)])[None, :]
    ok, msg, ratio = scenes.rounding_regime(pose(tree), pose(exact), pose(wide), what)
    print(f"{msg}; error / bound {ratio:.3f}")
    assert ok, msg


@pytest.mark.parametrize("n,half", [(300, 6), (3500, 1)])
def test_direct_method_tree_mode_single_problem(ftk, contexts, n, half):
    """One problem, one level, one iteration: the pose (q, p) against the wide oracle; 3 500 features do not fit the LDS (the
    projection table in device memory)."""
    from tests.test_direct_method_gpu import CX, CY, FX, FY, scene
    rl, cl, uv, pts = scene(levels=1, n=n, half=half, rotation_deg=0.4, scale=1.004)
    K = [FX, FY, CX, CY]
    kw = dict(half=half, max_points=n, max_iteration=1)
    cpu = oracle_lib.direct_track(rl, cl, K, pts, uv, **kw)
    wide = oracle_lib.wide().direct_track(rl, cl, K, pts, uv, **kw)
    results = []
    for ctx in contexts:
        dm = ftk.DirectMethod(ctx)
        o = dm.options()
        o.kMaxTrackPointsNumber, o.kMaxIteration, o.kPatchRowHalfSize, o.kPatchColHalfSize = n, 1, half, half
        rp, cp = ftk.ImagePyramid.from_host_levels(rl, ctx), ftk.ImagePyramid.from_host_levels(cl, ctx)
        ok, c, q, p, s = dm.TrackFeatures(rp, cp, K, pts, uv)
        assert ok and dm.last_iterations == 1
        results.append((c, q, p, s))
    (c_t, q_t, p_t, s_t), (c_e, q_e, p_e, s_e) = results
    assert np.array_equal(q_e.view(np.uint32), cpu[2].view(np.uint32)) and np.array_equal(p_e.view(np.uint32), cpu[3].view(np.uint32))
    # one iteration projects with the pose it starts from: positions and statuses are the oracle's in both modes
    for c, s in ((c_t, s_t), (c_e, s_e)):
        assert np.array_equal(c.view(np.uint32), cpu[1].view(np.uint32)) and np.array_equal(s, cpu[4])
    _direct_regime((q_t, p_t), (cpu[2], cpu[3]), (wide[2], wide[3]), f"direct n={n}")
    dm = ftk.DirectMethod(contexts[0])
    o = dm.options()
    o.kMaxTrackPointsNumber, o.kMaxIteration, o.kPatchRowHalfSize, o.kPatchColHalfSize = n, 1, half, half
    again = dm.TrackFeatures(ftk.ImagePyramid.from_host_levels(rl, contexts[0]), ftk.ImagePyramid.from_host_levels(cl, contexts[0]), K, pts, uv)
    assert np.array_equal(again[2].view(np.uint32), q_t.view(np.uint32)) and np.array_equal(again[3].view(np.uint32), p_t.view(np.uint32))


def test_direct_method_tree_mode_batch(ftk):
    """DeviceDirectBatch in the tree mode: every problem's pose against the wide oracle run on that problem alone."""
    import torch
    from feature_tracker_amd import device as D
    from tests.test_direct_method_gpu import CX, CY, FX, FY, scene
    sizes = (300, 1, 120, 37, 260)
    rl, cl, uv_all, pts_all = scene(n=max(sizes), levels=1)
    K = [FX, FY, CX, CY]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        ctx = D.context_on_stream(stream, 0)
        ctx.set_reduction("tree")
        rp, cp = D.upload_pyramid(rl, ctx, dev), D.upload_pyramid(cl, ctx, dev)
        problems, host = [], []
        for k, n in enumerate(sizes):
            uv, pts = np.ascontiguousarray(uv_all[k:k + n]), np.ascontiguousarray(pts_all[k:k + n])
            host.append((uv, pts))
            problems.append(dict(ref=rp, cur=cp, K=K, p_c_in_ref=torch.from_numpy(pts).to(dev).reshape(-1, 3),
                                 ref_uv=torch.from_numpy(uv).to(dev).reshape(-1, 2), cur_uv=torch.from_numpy(uv.copy()).to(dev).reshape(-1, 2),
                                 pose=torch.tensor([1, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=dev),
                                 status=torch.zeros(n, dtype=torch.uint8, device=dev), status_valid=False,
                                 iterations=torch.zeros(1, dtype=torch.int32, device=dev)))
        opt = ftk.DirectMethodOptions()
        opt.kMaxTrackPointsNumber, opt.kMaxIteration = 500, 1
        D.DeviceDirectBatch(opt, problems, ctx).track()
        stream.synchronize()
    for (uv, pts), pr in zip(host, problems):
        cpu = oracle_lib.direct_track(rl, cl, K, pts, uv, max_points=500, max_iteration=1)
        wide = oracle_lib.wide().direct_track(rl, cl, K, pts, uv, max_points=500, max_iteration=1)
        pose = pr["pose"].cpu().numpy()
        assert np.array_equal(pr["cur_uv"].cpu().numpy().view(np.uint32), cpu[1].view(np.uint32))
        assert np.array_equal(pr["status"].cpu().numpy(), cpu[4]) and int(pr["iterations"].cpu().numpy()[0]) == 1
        if len(uv) >= 6:  # (fewer features than pose parameters: singular normal equations, the step is rounding noise)
            _direct_regime((pose[:4], pose[4:]), (cpu[2], cpu[3]), (wide[2], wide[3]), f"direct batch problem of {len(uv)}")
        else:
            assert np.isfinite(pose).all()
    ctx.close()


# ---- 3. what the tree mode leaves exact ------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_affine_inverse_and_direct_stay_exact_under_tree_mode(ftk, contexts, switch, shape):
    """include/ftk.h: the non-fast affine variants ignore the setting.  Full tracking (15 iterations), one level, every shape."""
    _, hr, hc, _, _, _, n = shape
    ref_levels, cur_levels = scenes.scene(320, 240, 1, "easy", "similarity")
    uv = scenes.features(n, 320, 240, half=min(max(hr, hc), 20))
    pin(switch, shape)
    for method in ("inverse", "direct"):
        cpu = oracle_track(oracle_lib, "affine", method, ref_levels, cur_levels, uv, hr, hc, max_iteration=15)
        gpu = track(ftk, contexts[0], "affine", method, ref_levels, cur_levels, uv, hr, hc, max_iteration=15)
        assert_bits(gpu, cpu, f"tree affine/{method} {shape[0]}")


@pytest.mark.parametrize("model,method,half,force", [("basic", "inverse", 33, None), ("affine", "direct", 19, None), ("lssd", "fast", 33, None),
                                                     ("basic", "fast", 6, "1"), ("basic", "inverse", 6, "1"), ("lssd", "inverse", 6, "1"),
                                                     ("affine", "fast", 6, "2"), ("lssd", "fast", 6, "1"), ("basic", "direct", 6, "2")])
def test_large_patch_form_stays_exact_under_tree_mode(ftk, contexts, switch, model, method, half, force):
    """The large-patch (spill) form forces p.tree = 0 (klt_plan.cpp): by itself from beyond a workgroup's LDS, and forced with
    FTK_KLT_SPILL on an ordinary patch.  Full multi-level tracking, bit for bit."""
    switch("FTK_KLT_SPILL", force)
    ref_levels, cur_levels = scenes.scene(640, 480, 2, "easy", "similarity")
    uv = scenes.features(24 if half > 10 else 150, 640, 480, half=min(half, 20), border_fraction=0.1)
    cpu = oracle_track(oracle_lib, model, method, ref_levels, cur_levels, uv, half, max_iteration=15)
    gpu = track(ftk, contexts[0], model, method, ref_levels, cur_levels, uv, half, max_iteration=15)
    assert_bits(gpu, cpu, f"tree spill {model}/{method} half={half} force={force}")
