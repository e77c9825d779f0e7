"""DenseOpticalFlow (Farneback) on the device against the scalar restatement (tests/dense_flow_ref.c): every case is
bit-identical on both flow planes (any NaN equals any NaN)."""
import os
import subprocess

import numpy as np
import pytest

from feature_tracker_amd import synth
from tests import dense_flow_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "data", "optical_flow")


def example_pair():
    from PIL import Image
    ref = np.array(Image.open(os.path.join(DATA, "ref_image.png")).convert("L"))
    cur = np.array(Image.open(os.path.join(DATA, "cur_image.png")).convert("L"))
    return ref, cur


def flow_object(ftk, ctx, **opts):
    d = ftk.DenseOpticalFlow(ctx)
    for name, value in opts.items():
        setattr(d.options(), name, value)
    return d


def ref_options(d):
    o = d.options()
    return R.options(o.kMaxIteration, o.kHalfPatchSize, o.kMaxConvergeStep, o.kMaxDeltaFlowStep)


def check_pyramid(ftk, ctx, ref_levels, cur_levels, k=(0.0, 0.0, 0.0), **opts):
    d = flow_object(ftk, ctx, **opts)
    d._k = np.array(k, np.float32)
    ok, (fr, fc) = d.Track(ftk.ImagePyramid.from_host_levels(ref_levels, ctx), ftk.ImagePyramid.from_host_levels(cur_levels, ctx))
    ok_c, fr_c, fc_c, _ = R.track_pyramid(ref_levels, cur_levels, ref_options(d), k)
    assert ok and ok_c
    assert R.same(fr, fr_c), f"flow_r differs at {np.argwhere(fr.view(np.uint32) != fr_c.view(np.uint32))[:5].tolist()}"
    assert R.same(fc, fc_c), f"flow_c differs at {np.argwhere(fc.view(np.uint32) != fc_c.view(np.uint32))[:5].tolist()}"
    return fr, fc


def test_reference_program_workload(ftk, gpu_ctx):
    """test_dense_optical_flow.cpp's settings: the example pair (752 x 480), 5 levels, half patch 2, 20 iterations."""
    ref, cur = example_pair()
    assert ref.shape == (480, 752)
    check_pyramid(ftk, gpu_ctx, synth.build_pyramid(ref, 5), synth.build_pyramid(cur, 5), kHalfPatchSize=2, kMaxIteration=20)


@pytest.mark.parametrize("kind", ["translation", "similarity", "vga4"])
def test_defaults_on_synthetic_pairs(ftk, gpu_ctx, kind):
    if kind == "translation":
        ref, cur = synth.make_image_pair(320, 240, (2.6, -1.7))
        levels = 3
    elif kind == "similarity":
        ref, cur = synth.make_image_pair(320, 240, (1.3, 0.8), rotation_deg=2.0, scale=1.03)
        levels = 3
    else:
        ref, cur = synth.make_image_pair(640, 480, (3.3, -2.1))
        levels = 4
    check_pyramid(ftk, gpu_ctx, synth.build_pyramid(ref, levels), synth.build_pyramid(cur, levels))


@pytest.mark.parametrize("w,h,levels", [(333, 251, 3), (1, 1, 1), (3, 2, 1), (4, 5, 1)])
def test_odd_and_tiny_sizes(ftk, gpu_ctx, w, h, levels):
    ref, cur = synth.make_image_pair(max(w, 8), max(h, 8), (1.4, 0.6))
    ref, cur = np.ascontiguousarray(ref[:h, :w]), np.ascontiguousarray(cur[:h, :w])
    check_pyramid(ftk, gpu_ctx, synth.build_pyramid(ref, levels), synth.build_pyramid(cur, levels))


@pytest.mark.parametrize("half", [0, 1, 3, 7, 17])
def test_half_patch_values(ftk, gpu_ctx, half):
    """0 on a fresh object (k2 = k4 = k22 = 0), 1 .. 7, and 17 > the moments kernel's LDS bound (16: global reads)."""
    ref, cur = synth.make_image_pair(160, 120, (1.8, -1.2))
    check_pyramid(ftk, gpu_ctx, synth.build_pyramid(ref, 2), synth.build_pyramid(cur, 2), kHalfPatchSize=half)


def test_stale_k_quirk_through_the_class(ftk, gpu_ctx):
    """half patch 3, then 0 on the same object: the second call keeps the first call's k2 / k4 / k22 (:95-98).  (With a 1 x 1 window
    Sr = Sc = 0, so b = 0 and the flow does not move whatever k is; what the stale k changes is A, and the call still matches.)"""
    ref, cur = synth.make_image_pair(160, 120, (1.8, -1.2))
    rl, cl = synth.build_pyramid(ref, 2), synth.build_pyramid(cur, 2)
    d = flow_object(ftk, gpu_ctx, kHalfPatchSize=3)
    rp, cp = ftk.ImagePyramid.from_host_levels(rl, gpu_ctx), ftk.ImagePyramid.from_host_levels(cl, gpu_ctx)
    ok, _ = d.Track(rp, cp)
    _, _, _, k = R.track_pyramid(rl, cl, ref_options(d))
    d.options().kHalfPatchSize = 0
    ok2, (fr, fc) = d.Track(rp, cp)
    ok_c, fr_c, fc_c, _ = R.track_pyramid(rl, cl, ref_options(d), k)
    assert ok and ok2 and ok_c and np.all(k != 0)
    assert R.same(fr, fr_c) and R.same(fc, fc_c)
    assert np.array_equal(d._k, k)


def test_negative_half_patch(ftk, gpu_ctx):
    ref, cur = synth.make_image_pair(96, 64, (1.0, 1.0))
    d = flow_object(ftk, gpu_ctx, kHalfPatchSize=-1)
    ok, (fr, fc) = d.Track(ftk.ImagePyramid.from_host_levels(synth.build_pyramid(ref, 3), gpu_ctx),
                           ftk.ImagePyramid.from_host_levels(synth.build_pyramid(cur, 3), gpu_ctx))
    assert ok and fr.shape == (64, 96) and not fr.any() and not fc.any()
    init = [np.full((64, 96), 0.5, np.float32), np.full((64, 96), -0.5, np.float32)]
    ok, out = d.Track(ref, cur, init)
    assert not ok and out[0] is init[0] and out[1] is init[1]
    ok_c, _, _, _ = R.track_image(ref, cur, ref_options(d))
    assert not ok_c


def check_image(ftk, ctx, ref, cur, flow_r=None, flow_c=None, **opts):
    d = flow_object(ftk, ctx, **opts)
    ok, (fr, fc) = d.Track(ref, cur, [flow_r, flow_c])
    ok_c, fr_c, fc_c, _ = R.track_image(ref, cur, ref_options(d), (0.0, 0.0, 0.0), flow_r, flow_c)
    assert ok and ok_c
    assert R.same(fr, fr_c) and R.same(fc, fc_c)
    return fr, fc


def test_single_level_kept_random_initial_flow(ftk, gpu_ctx):
    ref, cur = synth.make_image_pair(200, 150, (2.2, -1.4))
    rs = np.random.RandomState(7)
    fr0 = rs.uniform(-5, 5, ref.shape).astype(np.float32)
    fc0 = rs.uniform(-5, 5, ref.shape).astype(np.float32)
    check_image(ftk, gpu_ctx, ref, cur, fr0, fc0)


def test_single_level_planes_reset_independently(ftk, gpu_ctx):
    ref, cur = synth.make_image_pair(120, 90, (1.2, 0.4))
    good = np.full(ref.shape, 0.75, np.float32)
    wrong = np.full((10, 10), 3.0, np.float32)
    fr_a, _ = check_image(ftk, gpu_ctx, ref, cur, good, wrong)
    _, fc_b = check_image(ftk, gpu_ctx, ref, cur, None, good)
    fr_z, fc_z = check_image(ftk, gpu_ctx, ref, cur, None, None)
    assert not R.same(fr_a, fr_z) and not R.same(fc_b, fc_z)


def test_single_level_hostile_initial_flows(ftk, gpu_ctx):
    """NaN, +-inf, -0.0 and 1e30 in the initial guess: no fault, and the restatement's answer (NaN where it gives NaN)."""
    ref, cur = synth.make_image_pair(64, 48, (1.0, -1.0))
    rs = np.random.RandomState(3)
    specials = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 1e30, -1e30, 3e9], np.float32)
    fr0 = rs.uniform(-3, 3, ref.shape).astype(np.float32)
    fc0 = rs.uniform(-3, 3, ref.shape).astype(np.float32)
    mask = rs.rand(*ref.shape) < 0.3
    fr0[mask] = rs.choice(specials, mask.sum())
    mask_c = rs.rand(*ref.shape) < 0.3
    fc0[mask_c] = rs.choice(specials, mask_c.sum())
    check_image(ftk, gpu_ctx, ref, cur, fr0, fc0)


def test_single_level_ref_and_cur_of_different_sizes(ftk, gpu_ctx):
    ref, _ = synth.make_image_pair(130, 97, (0.0, 0.0))
    _, cur = synth.make_image_pair(101, 120, (1.5, -0.5))
    check_image(ftk, gpu_ctx, ref, cur)
    check_image(ftk, gpu_ctx, cur, ref)


@pytest.mark.parametrize("opts", [dict(kMaxIteration=0), dict(kMaxIteration=1), dict(kMaxDeltaFlowStep=0.25), dict(kMaxConvergeStep=1e-3)])
def test_option_edges(ftk, gpu_ctx, opts):
    ref, cur = synth.make_image_pair(192, 144, (2.9, -1.1))
    check_pyramid(ftk, gpu_ctx, synth.build_pyramid(ref, 3), synth.build_pyramid(cur, 3), **opts)


def test_device_entry_and_graph_capture(ftk, gpu_ctx):
    import torch

    from feature_tracker_amd import device as D

    ref, cur = synth.make_image_pair(256, 192, (2.1, -1.3))
    rl, cl = synth.build_pyramid(ref, 3), synth.build_pyramid(cur, 3)
    d = flow_object(ftk, gpu_ctx)
    ok, (fr_h, fc_h) = d.Track(ftk.ImagePyramid.from_host_levels(rl, gpu_ctx), ftk.ImagePyramid.from_host_levels(cl, gpu_ctx))
    assert ok
    stream = torch.cuda.Stream()
    ctx = D.context_on_stream(stream)
    rp, cp = D.upload_pyramid(rl, ctx, "cuda"), D.upload_pyramid(cl, ctx, "cuda")
    torch.cuda.synchronize()
    out_r = torch.empty((192, 256), dtype=torch.float32, device="cuda")
    out_c = torch.empty_like(out_r)
    opt = ftk.DenseOpticalFlowOptions()
    with torch.cuda.stream(stream):
        D.dense_flow_device(ctx, opt, rp, cp, out_r, out_c)
    stream.synchronize()
    assert R.same(out_r.cpu().numpy(), fr_h) and R.same(out_c.cpu().numpy(), fc_h)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        D.dense_flow_device(ctx, opt, rp, cp, out_r, out_c)
    for _ in range(3):
        out_r.fill_(7.0)
        out_c.fill_(7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert R.same(out_r.cpu().numpy(), fr_h) and R.same(out_c.cpu().numpy(), fc_h)
    ctx.close()


def test_capture_without_resident_workspace_fails_cleanly(ftk):
    """A captured call whose workspace is not resident yet returns an error instead of allocating inside the capture."""
    import torch

    from feature_tracker_amd import _native
    from feature_tracker_amd import device as D

    ref, cur = synth.make_image_pair(64, 48, (1.0, 0.0))
    stream = torch.cuda.Stream()
    ctx = D.context_on_stream(stream)
    rp, cp = D.upload_pyramid([ref], ctx, "cuda"), D.upload_pyramid([cur], ctx, "cuda")
    out_r = torch.empty((48, 64), dtype=torch.float32, device="cuda")
    out_c = torch.empty_like(out_r)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    err = None
    try:
        with torch.cuda.graph(graph, stream=stream):
            try:
                D.dense_flow_device(ctx, ftk.DenseOpticalFlowOptions(), rp, cp, out_r, out_c)
            except _native.FtkError as e:
                err = e
    except Exception:
        pass  # an empty capture may be refused by torch; what matters is the library's answer
    assert err is not None and err.code == -4 and "captured" in str(err)
    ctx.close()


def test_dense_flow_cli_matches_the_restatement(tmp_path):
    exe = os.path.join(ROOT, "feature_tracker_amd", "host", "build", "dense_flow_cli")
    assert os.path.exists(exe), "make -C feature_tracker_amd/host builds dense_flow_cli"
    out_r, out_c = str(tmp_path / "r.f32"), str(tmp_path / "c.f32")
    res = subprocess.run([exe, os.path.join(DATA, "ref_image.png"), os.path.join(DATA, "cur_image.png"), out_r, out_c], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "Gunnar Farneback" in res.stdout
    ref, cur = example_pair()
    ok_c, fr_c, fc_c, _ = R.track_pyramid(synth.build_pyramid(ref, 5), synth.build_pyramid(cur, 5), R.options(max_iteration=20, half_patch=2))
    assert ok_c
    fr = np.fromfile(out_r, np.float32).reshape(ref.shape)
    fc = np.fromfile(out_c, np.float32).reshape(ref.shape)
    assert R.same(fr, fr_c) and R.same(fc, fc_c)
