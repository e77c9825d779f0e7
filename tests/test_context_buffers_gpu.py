"""The context's buffers (csrc/ftk_buffer.h) on the GPU: every test takes a FRESH context without warm-up, so that the workspaces
really are allocated, regrown (small call, large call, small call again) and released here, and compares with the oracles the
families' own tests use.  What a regrown block must keep: the fill pattern its kernels rely on (all ones for the Hamming keys,
zero for the NNFeatureMatcher keys), and the refusal to grow inside a stream capture."""
import numpy as np
import pytest

from feature_tracker_amd import synth
from tests import nn_match_ref as NR
from tests import scenes
from tests.test_direct_method_gpu import CX, CY, FX, FY, scene as direct_scene

pytestmark = pytest.mark.gpu

DEV = "cuda"


def brief_matcher(ftk, ctx, cls="BriefMatcher", max_dist=60.0):
    m = getattr(ftk, cls)(ctx)
    m.options().kMaxValidDescriptorDistance = max_dist
    m.options().kMaxValidPredictColDistance = 40
    m.options().kMaxValidPredictRowDistance = 40
    return m


def positions(n_ref, n_cur, perm, seed=11):
    rs = np.random.RandomState(seed)
    cur_uv = np.stack([rs.uniform(0, 640, n_cur), rs.uniform(0, 480, n_cur)], axis=1).astype(np.float32)
    pred_uv = np.stack([rs.uniform(0, 640, n_ref), rs.uniform(0, 480, n_ref)], axis=1).astype(np.float32)
    for j, i in enumerate(perm):  # ref i is predicted near cur j where the two are a true pair
        if 0 <= i < n_ref:
            pred_uv[i] = cur_uv[j] + rs.uniform(-30, 30, 2).astype(np.float32)
    return pred_uv, cur_uv


def test_regrown_matcher_workspaces_keep_their_fill_pattern(ftk, oracle):
    """BRIEF-256 ForceMatch / NearbyMatch with n_ref 33, 300, 33 (keys and boxes grow, then the first 33 keys of the larger block serve
    again), the device entry with 3-word descriptors at 33 then 300 rows (the pad buffer grows), cosine ForceMatch at 20 then 300 rows."""
    import torch
    from feature_tracker_amd import device as D
    ctx = ftk.Context()
    n_cur = 40
    for n_ref in (33, 300, 33):
        ref, cur, perm = synth.make_descriptors(n_ref, n_cur, n_bits=256, flips=20)
        m = brief_matcher(ftk, ctx)
        ok_g, idx_g = m.ForceMatch(ref, cur)
        ok_c, idx_c = oracle.force_match(ref, cur, 60.0)
        assert ok_g and ok_c and np.array_equal(idx_g, idx_c), n_ref
        assert (idx_c >= 0).sum() > 0
        pred_uv, cur_uv = positions(n_ref, n_cur, perm)
        ok_g, idx_g = m.NearbyMatch(ref, cur, pred_uv, cur_uv)
        ok_c, idx_c = oracle.nearby_match(ref, cur, pred_uv, cur_uv, 60.0, max_col=40, max_row=40)
        assert ok_g == ok_c and np.array_equal(idx_g, idx_c), n_ref
    ctx.close()
    stream = torch.cuda.Stream()
    ctx = D.context_on_stream(stream)
    with torch.cuda.stream(stream):
        for n_ref in (33, 300):  # 96 bits = 3 words: padded to 4 in a context-owned copy
            ref, cur, _ = synth.make_descriptors(n_ref, n_cur, n_bits=96, flips=7)
            d_ref = torch.from_numpy(ftk.pack_brief(ref).view(np.int32)).to(DEV)
            d_cur = torch.from_numpy(ftk.pack_brief(cur).view(np.int32)).to(DEV)
            assert d_ref.shape[1] == 3
            d_idx = torch.full((n_ref,), -1, dtype=torch.int32, device=DEV)
            D.hamming_match_device(ctx, d_ref, d_cur, 96, 25.0, d_idx)
            stream.synchronize()
            ok_c, idx_c = oracle.force_match(ref, cur, 25.0)
            assert np.array_equal(d_idx.cpu().numpy(), idx_c), n_ref
            assert (idx_c >= 0).sum() > 0
    ctx.close()
    ctx = ftk.Context()
    for n_ref in (20, 300):
        ref, cur, _ = synth.make_float_descriptors(n_ref, n_cur, dim=128)
        ok_g, idx_g = brief_matcher(ftk, ctx, "CosineMatcher", 0.6).ForceMatch(ref, cur)
        ok_c, idx_c = oracle.match_float(ref, cur, 0.6)
        assert ok_g and ok_c and np.array_equal(idx_g, idx_c), n_ref
    ctx.close()


def test_regrown_nn_keys_are_clean(ftk):
    """nn_match_scores on 8 x 8, 200 x 200, 8 x 8 scores: the key workspace grows once, zero-filled, and serves the small call again."""
    ctx = ftk.Context()
    m = ftk.NNFeatureMatcher(ctx)
    m.options().kMinValidMatchScore = 0.2
    rng = np.random.default_rng(5)
    for n in (8, 200, 8):
        scores = NR.quantised(rng, (n, n))
        ok, idx, st = m.match_scores(scores)
        want_idx, want_st = NR.match_scores(scores, 0.2)
        assert ok and np.array_equal(idx, want_idx) and np.array_equal(st, want_st), n
    ctx.close()


def direct_batch(ftk, oracle, ctx, stream, rl, cl, rp, cp, uv_all, pts_all, n_problems):
    import torch
    from feature_tracker_amd import device as D
    problems, host = [], []
    for k in range(n_problems):
        uv, pts = np.ascontiguousarray(uv_all[k:]), np.ascontiguousarray(pts_all[k:])
        host.append((uv, pts))
        problems.append(dict(ref=rp, cur=cp, K=[FX, FY, CX, CY], p_c_in_ref=torch.from_numpy(pts).to(DEV), ref_uv=torch.from_numpy(uv).to(DEV),
                             cur_uv=torch.from_numpy(uv.copy()).to(DEV), pose=torch.tensor([1, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=DEV),
                             status=torch.zeros(len(uv), dtype=torch.uint8, device=DEV), status_valid=False,
                             iterations=torch.zeros(1, dtype=torch.int32, device=DEV)))
    D.DeviceDirectBatch(ftk.DirectMethodOptions(), problems, ctx).track()
    stream.synchronize()
    for (uv, pts), pr in zip(host, problems):
        ok, c, q, p, st, it = oracle.direct_track(rl, cl, [FX, FY, CX, CY], pts, uv)
        pose = pr["pose"].cpu().numpy()
        assert np.array_equal(pose[:4].view(np.uint32), np.float32(q).view(np.uint32)) and np.array_equal(pose[4:].view(np.uint32), np.float32(p).view(np.uint32))
        assert np.array_equal(pr["cur_uv"].cpu().numpy().view(np.uint32), c.view(np.uint32))
        assert np.array_equal(pr["status"].cpu().numpy(), st)
        assert int(pr["iterations"].cpu().numpy()[0]) == it


def test_direct_problem_table_grows_and_is_reused(ftk, oracle):
    """Batches of 1, 3 and 1 direct-method problems (about 20 features on a 64 x 64 pair) on one context: the problem table and the
    spread workspace grow for the second batch and serve the third; every problem equals the oracle run on it alone."""
    import torch
    from feature_tracker_amd import device as D
    rl, cl, uv, pts = direct_scene(w=64, h=64, levels=2, n=20, shift=(1.3, -0.8))
    stream = torch.cuda.Stream()
    ctx = D.context_on_stream(stream)
    with torch.cuda.stream(stream):
        rp, cp = D.upload_pyramid(rl, ctx, DEV), D.upload_pyramid(cl, ctx, DEV)
        for n_problems in (1, 3, 1):
            direct_batch(ftk, oracle, ctx, stream, rl, cl, rp, cp, uv, pts, n_problems)
    ctx.close()


def test_large_patch_slices_are_not_allocated_inside_a_capture(ftk, oracle):
    """A fresh context's first large-patch tracker call (half 19: the smallest of test_patches_beyond_a_workgroups_lds_run_the_large_patch_form)
    inside a stream capture returns FTK_E_UNSUPPORTED and allocates nothing; the same call outside the capture equals the oracle."""
    import torch
    from feature_tracker_amd import _native
    from feature_tracker_amd import device as D
    ref_levels, cur_levels = scenes.scene(640, 480, 2)
    uv = scenes.features(24, 640, 480, half=19, border_fraction=0.1)
    stream = torch.cuda.Stream()
    ctx = D.context_on_stream(stream)
    opt = ftk.OpticalFlowOptions()
    opt.kMethod, opt.kPatchRowHalfSize, opt.kPatchColHalfSize, opt.kMaxTrackPointsNumber = "direct", 19, 19, 100000
    with torch.cuda.stream(stream):
        klt = D.DeviceKlt("affine", opt, D.upload_pyramid(ref_levels, ctx, DEV), D.upload_pyramid(cur_levels, ctx, DEV), ctx)
        d_ref = torch.from_numpy(uv).to(DEV)
        d_in, d_out = d_ref.clone(), torch.empty_like(d_ref)
        d_st, d_so = torch.zeros(len(uv), dtype=torch.uint8, device=DEV), torch.empty(len(uv), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    err = None
    try:
        with torch.cuda.graph(graph, stream=stream):
            try:
                klt.track(d_ref, d_in, d_st, d_out, d_so)
            except _native.FtkError as e:
                err = e
    except Exception:
        pass  # an empty capture may be refused by torch; what matters is the library's answer
    assert err is not None and err.code == -4 and "captured" in str(err)
    with torch.cuda.stream(stream):
        klt.track(d_ref, d_in, d_st, d_out, d_so)
        stream.synchronize()
    ok, c, s, _ = oracle.klt_track_pyramid("affine", ref_levels, cur_levels, uv, method="direct", half=19)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), c.view(np.uint32)) and np.array_equal(d_so.cpu().numpy(), s)
    ctx.close()


def small_calls_of_every_family(ftk, ctx, data):
    """Pyramid build, one tracker, BRIEF, Harris, both matchers, the direct method, dense flow, the nn scores, the RAFT build."""
    import torch
    from feature_tracker_amd import _native
    from feature_tracker_amd import device as D
    uv = data["uv"]
    assert ftk.ImagePyramid.build(data["rl"][0], 2, ctx).level() == 2
    rp, cp = ftk.ImagePyramid.from_host_levels(data["rl"], ctx), ftk.ImagePyramid.from_host_levels(data["cl"], ctx)
    klt = ftk.OpticalFlowBasicKlt(ctx)
    klt.options().kMethod = "inverse"
    out = {"klt": klt.TrackFeatures(rp, cp, uv)}
    words = ftk.BriefDescriptor(ctx).compute_packed(rp, uv)
    assert words.shape == (len(uv), 8)
    harris = ftk.FeaturePointHarrisDetector(ctx)
    assert harris.DetectGoodFeatures(rp, 10)[0]
    out["hamming"] = brief_matcher(ftk, ctx).ForceMatch(data["bits_ref"], data["bits_cur"])
    out["cosine"] = brief_matcher(ftk, ctx, "CosineMatcher", 0.6).ForceMatch(data["f_ref"], data["f_cur"])
    dm = ftk.DirectMethod(ctx)
    assert dm.TrackFeatures(rp, cp, [FX, FY, CX, CY], data["pts"], data["duv"], None, (1, 0, 0, 0), (0, 0, 0), None)[0]
    assert ftk.DenseOpticalFlow(ctx).Track(rp, cp)[0]
    m = ftk.NNFeatureMatcher(ctx)
    m.options().kMinValidMatchScore = 0.2
    out["nn"] = m.match_scores(data["scores"])
    f0 = torch.from_numpy(data["fmap"]).to(DEV)
    volume = torch.empty(_native.corr_pyramid_layout(1, 4, 4, 1)[0], dtype=torch.float32, device=DEV)
    D.corr_pyramid_build_device(ctx, f0, f0, 1, volume)
    torch.cuda.synchronize()
    return out


def test_contexts_come_and_go(ftk, oracle):
    """Twenty contexts in one process, each making the smallest call of every family before it is destroyed (every buffer goes with
    its context: nothing is freed by name); a fresh context afterwards still reproduces the oracles."""
    rl, cl, duv, pts = direct_scene(w=64, h=64, levels=2, n=20, shift=(1.3, -0.8))
    rng = np.random.default_rng(9)
    bits_ref, bits_cur, _ = synth.make_descriptors(12, 16, n_bits=256, flips=20)
    f_ref, f_cur, _ = synth.make_float_descriptors(12, 16, dim=32)
    data = dict(rl=rl, cl=cl, uv=duv, duv=duv, pts=pts, bits_ref=bits_ref, bits_cur=bits_cur, f_ref=f_ref, f_cur=f_cur,
                scores=NR.quantised(rng, (8, 8)), fmap=rng.standard_normal((1, 4, 4, 4), dtype=np.float32))
    for _ in range(20):
        ctx = ftk.Context()
        small_calls_of_every_family(ftk, ctx, data)
        ctx.close()
    ctx = ftk.Context()
    out = small_calls_of_every_family(ftk, ctx, data)
    ctx.close()
    ok, c, s = out["klt"]
    ok_c, c_c, s_c, _ = oracle.klt_track_pyramid("basic", rl, cl, duv, method="inverse", half=6)
    assert ok == ok_c and np.array_equal(c.view(np.uint32), c_c.view(np.uint32)) and np.array_equal(s, s_c)
    assert np.array_equal(out["hamming"][1], oracle.force_match(bits_ref, bits_cur, 60.0)[1])
    assert np.array_equal(out["cosine"][1], oracle.match_float(f_ref, f_cur, 0.6)[1])
    want_idx, want_st = NR.match_scores(data["scores"], 0.2)
    assert out["nn"][0] and np.array_equal(out["nn"][1], want_idx) and np.array_equal(out["nn"][2], want_st)
