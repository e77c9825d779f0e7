"""DenseOpticalFlow's HIP kernels against ref64 (tests/dense_ref64.py) directly, with the cases, the criteria and the tolerances of
tests/test_dense_ref64_cpu.py - not routed through the C restatement - in every form the product has:
* ftk.DenseOpticalFlow().Track(pyramid, pyramid) and Track(image, image, init) through the host class: every one-step case (the
  16 x 16, 17 x 15, 33 x 17, 97 x 61, one-row and one-column images, ref and cur of different sizes in both orders, so that one
  image's tiles of the two-image moments grid leave early; samples off every edge; the cap binding; half patch 0, 1, 16 (moments
  from LDS) and 17 (from global memory)), the kMaxIteration = 0 median cases, the upsample case and every end-to-end case (a
  3-level pyramid whose top level is smaller than the window among them);
* device.dense_flow_device on a torch stream with device-resident pyramids and outputs: every case that form can express (it has
  no initial flow: the pyramid cases, the image cases that start from zero as a one-level pyramid, the zero-field one-step cases
  and the upsample case).
The stability mask of the end-to-end cases is ref64's own (stable_mask), computed before the kernels run.

Each test prints its figures ("DENSE gpu vs ref64 ...").  The kernels are bit-identical to the C restatement
(tests/test_dense_flow_gpu.py), so on the cases both run the figures to expect are those of tests/test_dense_ref64_cpu.py: one step
8.5e-4 px, upsample 2.0e-4 px, end to end 8.5e-3 px on the stable pixels.  This module's own figures on an MI355X have not been
recorded here yet.
"""
import numpy as np
import pytest

from tests import dense_ref64 as R64
from tests.test_dense_ref64_cpu import (E2E_CASES, MEDIAN_CASES, STEP_CASES, TOL_E2E, TOL_STEP, check_e2e, check_median, check_step,
                                        check_upsample)

pytestmark = pytest.mark.gpu


class HostClass:
    """ftk.DenseOpticalFlow: both Track overloads."""
    name = "host class"

    def __init__(self, ftk, ctx):
        self.ftk, self.ctx = ftk, ctx

    def _object(self, opt, k):
        d = self.ftk.DenseOpticalFlow(self.ctx)
        o = d.options()
        o.kMaxIteration, o.kHalfPatchSize = opt.kMaxIteration, opt.kHalfPatchSize
        o.kMaxConvergeStep, o.kMaxDeltaFlowStep = opt.kMaxConvergeStep, opt.kMaxDeltaFlowStep
        d._k = np.array(k, np.float32)
        return d

    def image(self, ref, cur, fr0, fc0, opt, k):
        ok, out = self._object(opt, k).Track(ref, cur, [fr0, fc0])
        assert ok
        return out[0], out[1]

    def pyramid(self, rl, cl, opt, k):
        P = self.ftk.ImagePyramid
        ok, out = self._object(opt, k).Track(P.from_host_levels(rl, self.ctx), P.from_host_levels(cl, self.ctx))
        assert ok
        return out[0], out[1]

    def expresses(self, init):
        return True


class DeviceEntry:
    """device.dense_flow_device on a torch stream: pyramids and outputs resident on the device."""
    name = "device entry"

    def __init__(self, ftk):
        import torch
        from feature_tracker_amd import device as D
        self.ftk, self.torch, self.D = ftk, torch, D
        self.stream = torch.cuda.Stream()
        self.ctx = D.context_on_stream(self.stream)

    def close(self):
        self.ctx.close()

    def expresses(self, init):
        return all(f is None or not np.any(f) for f in init)

    def pyramid(self, rl, cl, opt, k):
        torch, D = self.torch, self.D
        rp, cp = D.upload_pyramid(rl, self.ctx, "cuda"), D.upload_pyramid(cl, self.ctx, "cuda")
        torch.cuda.synchronize()
        out_r = torch.full(rl[0].shape, 7.0, dtype=torch.float32, device="cuda")
        out_c = torch.full(rl[0].shape, 7.0, dtype=torch.float32, device="cuda")
        o = self.ftk.DenseOpticalFlowOptions()
        o.kMaxIteration, o.kHalfPatchSize = opt.kMaxIteration, opt.kHalfPatchSize
        o.kMaxConvergeStep, o.kMaxDeltaFlowStep = opt.kMaxConvergeStep, opt.kMaxDeltaFlowStep
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            D.dense_flow_device(self.ctx, o, rp, cp, out_r, out_c, k)
        self.stream.synchronize()
        return out_r.cpu().numpy(), out_c.cpu().numpy()

    def image(self, ref, cur, fr0, fc0, opt, k):
        assert self.expresses((fr0, fc0)) and np.shape(fr0) in ((), ref.shape), "the device entry has no initial flow"
        return self.pyramid([ref], [cur], opt, k)


@pytest.fixture
def forms(ftk, gpu_ctx):
    entry = DeviceEntry(ftk)
    yield {"host": HostClass(ftk, gpu_ctx), "device": entry}
    entry.close()


@pytest.mark.parametrize("form", ["host", "device"])
def test_one_step_teacher_forced(forms, form):
    run = forms[form]
    fig = {name: check_step(run, name) for name, c in STEP_CASES.items() if run.expresses(c["F"])}
    assert len(fig) == (len(STEP_CASES) if form == "host" else 2)
    name = max(fig, key=fig.get)
    print(f"\nDENSE gpu vs ref64, {run.name}, one step: {len(fig)} cases, worst |d| {fig[name]:.3g} px ({name}); tolerance {TOL_STEP}")


@pytest.mark.parametrize("half", [0, 1, 16, 17])
def test_moments_from_lds_and_from_global_memory(forms, half):
    """Half patch 16 is the largest staged in LDS (kLdsHalf, dense_flow_kernels.hip), 17 the first read from global memory; 0 and 1
    are the smallest windows."""
    lds_half = 16
    fig = {name: check_step(forms["host"], name) for name in (f"half{half}", f"half{half}-off-edges")}
    print(f"\nDENSE gpu vs ref64, moments {'from LDS' if half <= lds_half else 'from global memory'}, half {half}: worst |d| "
          f"{max(fig.values()):.3g} px; tolerance {TOL_STEP}")


def test_zero_iterations_is_the_median_by_value(forms):
    for name in MEDIAN_CASES:
        check_median(forms["host"], name)


@pytest.mark.parametrize("form", ["host", "device"])
def test_upsample_then_one_step(forms, form):
    print(f"\nDENSE gpu vs ref64, {forms[form].name}, upsample + one step: worst |d| {check_upsample(forms[form]):.3g} px; tolerance {TOL_STEP}")


@pytest.mark.parametrize("form", ["host", "device"])
def test_end_to_end_where_ref64_is_stable(forms, form):
    run = forms[form]
    fig = {}
    for name, c in E2E_CASES.items():
        if c["form"] == "pyramid" or run.expresses(c["init"]):
            fig[name] = check_e2e(run, name)
    assert len(fig) == (len(E2E_CASES) if form == "host" else len(E2E_CASES) - 2)
    name = max(fig, key=lambda n: fig[n][0])
    print(f"\nDENSE gpu vs ref64, {run.name}, end to end: {len(fig)} cases, worst stable |d| {fig[name][0]:.3g} px ({name}), largest masked "
          f"share {max(f[1] for f in fig.values()):.2%}, worst masked |d| {max(f[3] for f in fig.values()):.3g} px; tolerance {TOL_E2E}")


def test_device_entry_stale_k_reaches_the_kernel(forms):
    """Half patch 0 with a stale k through the device entry's k_moments: b = 0 whatever k is, so the field does not move and the
    result is the median of the zero field; what the call must not do is fail or read k as a half patch's own."""
    c = STEP_CASES["half0-stale-k"]
    fr, fc = forms["device"].pyramid([c["ref"]], [c["cur"]], c["opt"], c["k"])
    _, want, _ = R64.track_image(c["ref"], c["cur"], (None, None), c["opt"], c["k"])
    assert np.abs(fr - want[0]).max() <= TOL_STEP and np.abs(fc - want[1]).max() <= TOL_STEP
