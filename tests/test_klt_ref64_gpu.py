"""The HIP trackers against ref64 (tests/klt_ref64.py) directly, with the criteria and cases of tests/test_klt_ref64_cpu.py — not
routed through the oracle.  Also the launch forms that exist only on the device, pinned with the library's switches: the pipelined
Basic-inverse kernel (the default Basic-inverse launch), one-wave and multi-wave fast kernels, the large-patch form and the
chunked LSSD-fast level.  Measured: 26 tests in about 15 s on one MI355X host, most of it ref64 on the host CPU."""
import numpy as np
import pytest

from tests import scenes
from tests.test_klt_gpu import make_tracker
from tests.test_klt_ref64_cpu import (VARIANTS, VARIANT_IDS, check_full_variant, check_one_step_variant, full_check, run_ref,
                                      _cases)

pytestmark = pytest.mark.gpu

_OPT = {"max_iteration": "kMaxIteration", "max_large_step": "kMaxToleranceLargeStep", "converge": "kMaxConvergeStep"}


def gpu_runner(ftk):
    def run(kind, model, method, lum, case, prior):
        name, ri, ci, uv, cur, st, opt = case
        opt = dict(opt)
        kw = {_OPT[k]: opt.pop(k) for k in list(opt) if k in _OPT}
        if kind.startswith("one"):
            kw["kMaxIteration"] = 1
        klt = make_tracker(ftk, model, method, opt.get("half", 6), opt.get("half_cols"), max_points=opt.get("max_points", 100000), **kw)
        if prior is not None:
            if model == "affine":
                klt.predict_affine = np.asarray(prior, np.float32)
            else:
                klt.predict_R_cr = np.asarray(prior, np.float32)
        if model == "lssd":
            klt.consider_patch_luminance = lum
        if kind == "one":
            ok, c, s = klt.TrackFeatures(ri, ci, uv, cur, st)
        else:
            levels = ([ri], [ci]) if kind == "one-pyr" else (ri, ci)
            ok, c, s = klt.TrackFeatures(ftk.ImagePyramid.from_host_levels(levels[0]), ftk.ImagePyramid.from_host_levels(levels[1]),
                                         uv, cur, st)
        assert ok
        return c, s, klt.last_iterations
    return run


@pytest.mark.parametrize("model,method,lum", VARIANTS, ids=VARIANT_IDS)
def test_one_step_kernels_match_ref64(ftk, model, method, lum):
    agg = check_one_step_variant(gpu_runner(ftk), model, method, lum)
    print(f"\nONE-STEP gpu {model}/{method}{' luminance' if lum else ''}: {agg}")


@pytest.mark.parametrize("model,method,lum", VARIANTS, ids=VARIANT_IDS)
def test_full_tracking_kernels_match_ref64(ftk, model, method, lum):
    agg = check_full_variant(gpu_runner(ftk), model, method, lum)
    print(f"\nFULL gpu {model}/{method}{' luminance' if lum else ''}: {agg}")


LAUNCH_FORMS = {
    # one wave per feature, two features per workgroup: klt_fast_kernel's one-wave form and the chunked LSSD-fast level
    # (and the pipelined Basic-inverse kernel's one-wave packing)
    "one-wave": ({"FTK_KLT_WAVES": "1", "FTK_KLT_GROUP": "2", "FTK_LSSD_CHUNKED": "1"},
                 [(m, "fast", False) for m in ("basic", "affine", "lssd")] + [("lssd", "fast", True), ("basic", "inverse", False)]),
    # the generic kernel's multi-wave form for the fast variants, and the plain (unchunked) LSSD-fast level
    "multi-wave": ({"FTK_KLT_WAVES": "4", "FTK_LSSD_CHUNKED": "0"},
                   [(m, "fast", False) for m in ("basic", "affine", "lssd")] + [("lssd", "fast", True)]),
    # the large-patch form (per-pixel arrays in device memory) forced on ordinary patches
    "large-patch": ({"FTK_KLT_SPILL": "1"}, VARIANTS),
}


@pytest.mark.parametrize("form", sorted(LAUNCH_FORMS))
def test_launch_forms_match_ref64(ftk, switch, form):
    switches, variants = LAUNCH_FORMS[form]
    for k, v in switches.items():
        switch(k, v)
    run = gpu_runner(ftk)
    cases = [c for c in _cases("full") if c[0] in ("similarity-hard", "similarity-hard/rect, options, prediction, status")]
    for model, method, lum in variants:
        for case in cases:
            ref = run_ref("full", model, method, lum, case)
            c, s, it = run("full", model, method, lum, case, None)
            ok, msg, _, stats = full_check(model, ref, c, s, it, f"{form} {model}/{method} {case[0]}")
            assert ok, msg


@pytest.mark.parametrize("model,method,half", [("basic", "inverse", 45), ("affine", "inverse", 32), ("lssd", "fast", 36)])
def test_patches_beyond_a_workgroups_lds_match_ref64(ftk, model, method, half):
    """Halves beyond a workgroup's LDS run the large-patch form on their own."""
    ref_levels, cur_levels = scenes.scene(640, 480, 2)
    uv = scenes.features(24, 640, 480, half=half, border_fraction=0.1)
    case = ("large patch", ref_levels, cur_levels, uv, None, None, dict(half=half))
    ref = run_ref("full", model, method, False, case)
    c, s, it = gpu_runner(ftk)("full", model, method, False, case, None)
    ok, msg, _, stats = full_check(model, ref, c, s, it, f"half {half} {model}/{method}")
    assert ok and stats["compared"] > 0, msg
