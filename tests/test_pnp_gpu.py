"""PnpRansac on the device against the scalar restatement (tests/pnp_ref.c): pose, n_inliers, best, valid, status, counts and
models bit for bit at the sizes that cross the contract's edges (M = 5, 6, 7; the 256-point tile of the score kernel and of the summation
tree; five tiles with one point in the last; 65 536 points), at hypothesis counts that cross the 64-lane block and the 16-hypothesis group,
at every refit length, on the pose family, on hostile and degenerate inputs, repeated, replayed from a captured graph, and composed with
TwoViewRansac and TwoViewPose on the device."""
import numpy as np
import pytest

from tests import epipolar_ref as E
from tests import pnp_ref as R
from tests import two_view_pose_ref as P
from tests import two_view_ref as T

pytestmark = pytest.mark.gpu

ALL = R.OUTPUTS + R.HYPOTHESES


def _host(d_status, out, hypotheses=True):
    r = R.Result()
    r.status = d_status.cpu().numpy()
    for name in ("pose", "n_inliers", "best", "valid") + (R.HYPOTHESES if hypotheses else ()):
        setattr(r, name, getattr(out, name).cpu().numpy())
    return r


def _device(ftk, X, uv, status, solver=None, seed=None, **kw):
    import torch
    d_X, d_uv, d_status = torch.from_numpy(X).cuda(), torch.from_numpy(uv).cuda(), torch.from_numpy(status).cuda()
    solver = solver or ftk.PnpRansac(kw.pop("K", R.K), **kw)
    out = solver.solve(d_X, d_uv, d_status, seed=seed, return_hypotheses=True)
    torch.cuda.synchronize()
    assert E.same(d_X.cpu().numpy(), X) and E.same(d_uv.cpu().numpy(), uv)  # inputs other than status are untouched
    return _host(d_status, out)


@pytest.mark.parametrize("name", R.SIZE_CASES + ("zeros",))
def test_bit_identity_with_the_restatement(ftk, name):
    X, uv, status = R.case(name)
    want = R.solve(X, uv, status)
    assert int(want.valid[0]) == (-1 if name == "n5" else 1)
    assert R.same_results(_device(ftk, X, uv, status), want, ALL) == [], name


# (hypotheses, seed, the floor of the winner or -1 for none): at 2048 and 4096 a thread of the select kernel folds 2 and 4 hypotheses, and
# under these seeds the winner is a thread's second and third (best = 1987 and 3542), beyond the first 1024
HYPOTHESIS_COUNTS = [(1, 5, -1), (63, 5, -1), (64, 5, -1), (65, 5, -1), (512, 5, -1), (2048, 2, 1024), (4096, 3, 1024)]


@pytest.mark.parametrize("hypotheses, seed, floor", HYPOTHESIS_COUNTS, ids=[str(c[0]) for c in HYPOTHESIS_COUNTS])
def test_hypothesis_counts_across_the_block_and_the_group(ftk, hypotheses, seed, floor):
    X, uv, _, _ = R.scene(300, 2, noise=0.3, outlier_share=0.3)
    status = np.full(300, R.TRACKED, np.uint8)
    want = R.solve(X, uv, status, hypotheses=hypotheses, seed=seed)
    assert int(want.best[0]) >= floor
    assert R.same_results(_device(ftk, X, uv, status, hypotheses=hypotheses, seed=seed), want, ALL) == [], hypotheses


@pytest.mark.parametrize("refine", [0, 1, 4, 16])
def test_every_refit_length(ftk, refine):
    X, uv, _, _ = R.scene(300, 3, noise=0.3, outlier_share=0.3)
    status = np.full(300, R.TRACKED, np.uint8)
    want = R.solve(X, uv, status, refine_iterations=refine, seed=2)
    assert int(want.valid[0]) == 1 and want.trace[R.TRACE_STEPS] <= refine
    assert R.same_results(_device(ftk, X, uv, status, refine_iterations=refine, seed=2), want, ALL) == [], refine


FAMILY_CASES = ([(pose, n, 0.0, {}) for pose in R.SHEPPERD_POSES for n in (9, 257, 300)]
                + [(pose, 300, 0.3, dict(K=R.K_OTHER)) for pose in R.SHEPPERD_POSES])


def _family_id(case):
    pose, n, noise, kw = case
    return f"{pose}-n{n}" + ("-noise" if noise else "") + "".join(f"-{k}" for k in kw)


@pytest.mark.parametrize("case", FAMILY_CASES, ids=_family_id)
def test_bit_identity_on_a_pose_per_branch_of_the_quaternion(ftk, case):
    pose, n, noise, kw = case
    X, uv, status = R.family_case(pose, n, noise, K=kw.get("K", R.K))
    want = R.solve(X, uv, status, **kw)
    assert int(want.valid[0]) == 1 and want.trace[R.TRACE_SHEPPERD] == P.SHEPPERD_BRANCH[pose.split("/")[0]]
    assert R.same_results(_device(ftk, X, uv, status, **kw), want, ALL) == [], case


@pytest.mark.parametrize("name", R.HOSTILE_CASES)
def test_hostile_and_degenerate_inputs(ftk, name):
    X, uv, status = R.case(name)
    for threshold in (1.0, 0.0):
        want = R.solve(X, uv, status, threshold=threshold)
        assert R.same_results(_device(ftk, X, uv, status, threshold=threshold), want, ALL) == [], (name, threshold)


def test_a_repeated_call_gives_equal_bits(ftk):
    X, uv, status = R.case("n1025")
    solver = ftk.PnpRansac(R.K)
    first, second = _device(ftk, X, uv, status, solver), _device(ftk, X, uv, status, solver)
    assert R.same_results(first, second, ALL) == [] and R.same_results(first, R.solve(X, uv, status), ALL) == []
    small = R.case("n7")  # the workspace of the larger call, left as it is
    assert R.same_results(_device(ftk, *small, solver), R.solve(*small), ALL) == []


def test_a_captured_graph_replayed_on_changed_inputs_equals_the_eager_result(ftk):
    import torch
    X, uv, _, _ = R.scene(300, 2, noise=0.3, outlier_share=0.3)
    X2, uv2, _, _ = R.family_scene("y170/back", 300, 3, outlier_share=0.2)
    status = np.full(300, R.TRACKED, np.uint8)
    status2 = status.copy()
    status2[::5] = E.OUTSIDE
    solver = ftk.PnpRansac(R.K, threshold=0.5, seed=9)
    d_X, d_uv, d_status = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(uv.copy()).cuda(), torch.from_numpy(status.copy()).cuda()
    solver.solve(d_X, d_uv, d_status, return_hypotheses=True)  # the workspace is made here, outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = solver.solve(d_X, d_uv, d_status, return_hypotheses=True)
    d_X.copy_(torch.from_numpy(X2))
    d_uv.copy_(torch.from_numpy(uv2))
    d_status.copy_(torch.from_numpy(status2))
    graph.replay()
    torch.cuda.synchronize()
    got = _host(d_status, out)
    assert R.same_results(got, _device(ftk, X2, uv2, status2, threshold=0.5, seed=9), ALL) == []
    assert R.same_results(got, R.solve(X2, uv2, status2, threshold=0.5, seed=9), ALL) == []


def test_two_views_then_pnp_equals_the_three_restatements_composed(ftk):
    """TwoViewRansac("fundamental").filter on views 0 and 1, TwoViewPose.solve, then PnpRansac.solve on the landmarks and view 2, nothing
    read on the host in between; the pose of view 2 against ground truth up to the baseline's scale."""
    import torch
    from tests.test_pnp_cpu import COMPOSED_POSES, COMPOSED_ROTATION_TOLERANCE, COMPOSED_POSITION_TOLERANCE, composed_errors
    pose1, pose2 = (R.family_pose(name) for name in COMPOSED_POSES)
    uv0, uv1, uv2, _, _ = R.three_views(300, 1, pose1, pose2, noise=0.0, outlier_share=0.3)
    status = np.full(300, R.TRACKED, np.uint8)
    d0, d1, d2, d_status = (torch.from_numpy(a).cuda() for a in (uv0, uv1, uv2, status))
    ftk.TwoViewRansac("fundamental", hypotheses=512, threshold=1.0, seed=1).filter(d0, d1, d_status, E.IMAGE)
    pose01 = ftk.TwoViewPose(R.K, threshold=1.0).solve(d0, d1, d_status)
    d_status2 = d_status.clone()
    fit = ftk.PnpRansac(R.K, hypotheses=512, threshold=1.0, seed=3).solve(pose01.points, d2, d_status2, return_hypotheses=True)
    torch.cuda.synchronize()
    filtered = T.ransac(uv0, uv1, status, E.IMAGE, 1.0, 512, 1, "fundamental")
    want01 = P.solve(uv0, uv1, filtered.status)
    want = R.solve(want01.points, uv2, want01.status, seed=3)
    assert int(want01.valid[0]) == 1 and int(want.valid[0]) == 1 and int(want.n_inliers[0]) >= 150
    got = _host(d_status2, fit)
    assert E.same(pose01.points.cpu().numpy(), want01.points) and R.same_results(got, want, ALL) == []
    rotation, position = composed_errors(got.pose, pose1, pose2)
    print(f"view 2 against truth: rotation {rotation:.3e} rad, position {position:.3e}")
    assert rotation <= COMPOSED_ROTATION_TOLERANCE and position <= COMPOSED_POSITION_TOLERANCE


def test_the_context_stream_and_the_refusals_of_the_library(ftk):
    import torch
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    X, uv, status = R.case("n257")
    ctx = D.context_on_stream(torch.cuda.Stream())
    got = _device(ftk, X, uv, status, ftk.PnpRansac(R.K, ctx=ctx))
    assert R.same_results(got, R.solve(X, uv, status), ALL) == []
    lm = torch.zeros(16, 3, device="cuda")
    t = torch.zeros(16, 2, device="cuda")
    st = torch.ones(16, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(100000, dtype=torch.int64, device="cuda")
    o = torch.zeros(16, dtype=torch.int32, device="cuda")
    f = torch.zeros(64, device="cuda")
    call = lambda n=16, fx=500.0, cx=320.0, threshold=1.0, hypotheses=64, refine=4: N.lib().ftk_pnp_ransac_device(  # noqa: E731
        ctx.handle, None, lm.data_ptr(), t.data_ptr(), st.data_ptr(), n, fx, 500.0, cx, 240.0, threshold, hypotheses, refine, 0, ws.data_ptr(), f.data_ptr(),
        o.data_ptr(), o.data_ptr(), o.data_ptr(), None, None)
    inf, nan = float("inf"), float("nan")
    assert call(n=N.FTK_TRACK_TABLE_MAX_SLOTS + 1) == -4 and call(n=0) == -1  # FTK_E_UNSUPPORTED, FTK_E_INVALID_ARGUMENT: nothing launched
    assert call(hypotheses=0) == -1 and call(hypotheses=4097) == -4 and call(refine=-1) == -1 and call(refine=17) == -4
    assert call(fx=0.0) == -1 and call(fx=-1.0) == -1 and call(fx=nan) == -1 and call(fx=inf) == -1 and call(cx=nan) == -1 and call(fx=1e-50) == -1
    assert call(threshold=-1.0) == -1 and call(threshold=nan) == -1 and call(threshold=inf) == -1 and call(threshold=2.0e19) == -1
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == [1] * 16 and not f.any() and not o.any()


def test_a_wide_view_where_every_model_changes_sign(ftk):
    """R.wide_case: the elimination returns every null vector with the sample behind the camera, so the sign rule acts on all of them."""
    X, uv, status, _ = R.wide_case()
    want = R.solve(X, uv, status, K=R.K_WIDE)
    flipped = R.solve(X, uv, status, K=R.K_WIDE, variant=R.MUTANTS["sign_of_p_not_fixed"])
    assert int(want.valid[0]) == 1 and int(want.n_inliers[0]) == 64 and (want.models != flipped.models).any(1).sum() >= 400
    assert R.same_results(_device(ftk, X, uv, status, K=R.K_WIDE), want, ALL) == []
