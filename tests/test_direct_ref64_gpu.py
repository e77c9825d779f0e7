"""DirectMethod's HIP kernels against ref64 (tests/direct_ref64.py) directly, with the cases and the criterion of
tests/test_direct_ref64_cpu.py - not routed through the oracle - through ftk.DirectMethod().TrackFeatures / TrackFeaturesWorld, in
every launch form: the default dispatch (one problem spread over the chip), the one-workgroup kernel (FTK_DIRECT_SPREAD=0), three
producer workgroups whatever the size (FTK_DIRECT_SPREAD=3, FTK_DIRECT_SPREAD_MIN_TERMS=1), the tree reduction mode
(ftk_set_reduction_mode reaches DirectPlanInput::tree; it is not bit-identical to the oracle, so ref64 is its judge, at the same
bar), the feature table in device memory (the many-features case, in every form) and DeviceDirectBatch with problems of different
sizes, one batch per pyramid depth of 1, 2, 4 and 5 levels (a batch of mixed depths is refused, which is asserted).

Measured on one MI355X (each test prints its aggregate, "DIRECT gpu vs ref64 ..."), worst over the 68 comparable cases:
                                 worst pixel   worst induced pixel   worst |dp|   worst |dq|
  default, one-workgroup,
  three producers (identical)    1.6e-4 px     6.4e-4 px             1.9e-5       1.6e-6
  tree mode                      9.2e-5 px     6.7e-5 px             1.1e-6       9.9e-8
  device batches, 1/2/4/5 levels 1.6e-4 px     3.8e-5 px             5.9e-7       5.6e-8
The exact forms give the oracle's figures of tests/test_direct_ref64_cpu.py (they are bit-identical to it); the tree mode's sums
round less, which shows in the one-step cases.  9 tests in 3.6 s, most of it ref64 on the host.
"""
import numpy as np
import pytest

from tests.test_direct_ref64_cpu import batch_cases, check, check_all, comparable, run_ref

pytestmark = pytest.mark.gpu

FORMS = {
    "default": {},
    "one-workgroup": {"FTK_DIRECT_SPREAD": "0"},
    "spread-3-tiny": {"FTK_DIRECT_SPREAD": "3", "FTK_DIRECT_SPREAD_MIN_TERMS": "1"},
}


def gpu_runner(ftk, ctx=None):
    def run(c):
        dm = ftk.DirectMethod(ctx)
        o, opt = dm.options(), c["opt"]
        o.kMaxTrackPointsNumber = opt.get("max_points", 500)
        o.kMaxIteration = opt.get("max_iteration", 15)
        o.kPatchRowHalfSize = opt.get("half", 6)
        o.kPatchColHalfSize = opt.get("half_cols", opt.get("half", 6))
        o.kMaxConvergeStep = opt.get("converge", 1e-6)
        o.kMethod = opt.get("method", "direct")
        rp, cp = ftk.ImagePyramid.from_host_levels(c["rl"], ctx), ftk.ImagePyramid.from_host_levels(c["cl"], ctx)
        if c["world"] is not None:
            rq, rp_w = c["world"]
            ok, uv, q, p, st = dm.TrackFeaturesWorld(rp, cp, list(c["K"]), rq, rp_w, c["pts"], c["uv"], c["cur"], c["q"], c["p"], c["status"])
        else:
            ok, uv, q, p, st = dm.TrackFeatures(rp, cp, list(c["K"]), c["pts"], c["uv"], c["cur"], c["q"], c["p"], c["status"])
        return ok, uv, q, p, st, dm.last_iterations
    return run


@pytest.mark.parametrize("form", sorted(FORMS))
def test_kernels_match_ref64_in_every_launch_form(ftk, switch, form):
    for k, v in FORMS[form].items():
        switch(k, v)
    agg = check_all(gpu_runner(ftk))
    print(f"\nDIRECT gpu vs ref64, {form}: {agg}")


def test_tree_reduction_mode_matches_ref64(ftk):
    ctx = ftk.Context()
    try:
        ctx.set_reduction("tree")
        agg = check_all(gpu_runner(ftk, ctx))
    finally:
        ctx.close()
    print(f"\nDIRECT gpu vs ref64, tree mode: {agg}")


def _batch(ftk, cases, ctx_of):
    import torch
    from feature_tracker_amd import device as D
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        ctx = ctx_of(D, stream)
        problems = []
        for c in cases:
            n = len(c["uv"])
            rp, cp = D.upload_pyramid(c["rl"], ctx, dev), D.upload_pyramid(c["cl"], ctx, dev)
            problems.append(dict(ref=rp, cur=cp, K=list(c["K"]), p_c_in_ref=torch.from_numpy(c["pts"]).to(dev).reshape(-1, 3),
                                 ref_uv=torch.from_numpy(c["uv"]).to(dev).reshape(-1, 2), cur_uv=torch.from_numpy(c["uv"].copy()).to(dev).reshape(-1, 2),
                                 pose=torch.tensor([1, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=dev),
                                 status=torch.zeros(n, dtype=torch.uint8, device=dev), status_valid=False,
                                 iterations=torch.zeros(1, dtype=torch.int32, device=dev)))
        opt = ftk.DirectMethodOptions()
        opt.kMaxTrackPointsNumber = 500
        D.DeviceDirectBatch(opt, problems, ctx).track()
        stream.synchronize()
    out = []
    for pr in problems:
        pose = pr["pose"].cpu().numpy()
        out.append((True, pr["cur_uv"].cpu().numpy(), pose[:4], pose[4:], pr["status"].cpu().numpy(), int(pr["iterations"].cpu().numpy()[0])))
    return out


@pytest.mark.parametrize("levels", [1, 2, 4, 5])
def test_device_batches_of_different_sizes_match_ref64_problem_by_problem(ftk, levels):
    cases = batch_cases()[levels]
    got = _batch(ftk, cases, lambda D, stream: D.context_on_stream(stream, 0))
    worst = {}
    for c, g in zip(cases, got):
        ref = run_ref(c)
        assert not comparable(c, ref), c["name"]
        ok, msg, _, stats = check(c, ref, g)
        assert ok, msg
        for k in ("px", "induced", "dp", "dq"):
            worst[k] = max(worst.get(k, 0.0), stats[k])
    print(f"\nDIRECT gpu batch vs ref64, {levels} levels: {worst}")


def test_a_batch_of_mixed_pyramid_depths_is_refused(ftk):
    from feature_tracker_amd._native import FtkError
    cases = [batch_cases()[1][2], batch_cases()[2][2]]
    with pytest.raises(FtkError) as e:
        _batch(ftk, cases, lambda D, stream: D.context_on_stream(stream, 0))
    assert e.value.code == -4, e.value
