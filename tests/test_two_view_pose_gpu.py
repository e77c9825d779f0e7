"""TwoViewPose on the device against the scalar restatement (tests/two_view_pose_ref.c): pose, E, n_front, valid, n_points,
points and status bit for bit at the sizes that cross the contract's edges (M = 7, 8, 9; the 256-point tile of the summation tree; five tiles
with one point in the last; 65 536 points with 254 tiles in use, and with all 256 full), on hostile and degenerate inputs, repeated,
replayed from a captured graph, and composed with TwoViewRansac on the device."""
import numpy as np
import pytest

from tests import epipolar_ref as E
from tests import two_view_pose_ref as P
from tests import two_view_ref as T

pytestmark = pytest.mark.gpu


def _host(d_status, out):
    r = P.Result()
    r.status = d_status.cpu().numpy()
    for name in ("pose", "E", "n_front", "valid", "n_points", "points"):
        setattr(r, name, getattr(out, name).cpu().numpy())
    return r


def _device(ftk, ref, cur, status, solver=None, **kw):
    import torch
    d_ref, d_cur, d_status = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda(), torch.from_numpy(status).cuda()
    solver = solver or ftk.TwoViewPose(kw.pop("K", P.K), **kw)
    out = solver.solve(d_ref, d_cur, d_status)
    torch.cuda.synchronize()
    assert E.same(d_ref.cpu().numpy(), ref) and E.same(d_cur.cpu().numpy(), cur)  # inputs other than status are untouched
    return _host(d_status, out)


@pytest.mark.parametrize("name", ["n7", "n8", "n9", "n64_half", "n255", "n256", "n257", "n1025", "big65536", "full65536"])
def test_bit_identity_with_the_restatement(ftk, name):
    ref, cur, status = P.case(name)
    want = P.solve(ref, cur, status)
    assert int(want.valid[0]) == (-1 if name == "n7" else 1)
    assert P.same_results(_device(ftk, ref, cur, status), want) == [], name


# The pose family: every pose at 300 points (two tiles); a pose per branch of the quaternion at 9 and 257 points, through a
# second camera, and with 0.3 px noise at a 0.5 px threshold.  (pose, points, noise, arguments of the call)
FAMILY_CASES = ([(pose, 300, 0.0, {}) for pose in P.FAMILY] + [(pose, 9, 0.0, {}) for pose in P.SHEPPERD_POSES_N9]
                + [(pose, 257, 0.0, {}) for pose in P.SHEPPERD_POSES]
                + [(pose, 300, 0.0, dict(K_cur=P.K_OTHER)) for pose in P.SHEPPERD_POSES]
                + [(pose, 300, 0.3, dict(threshold=0.5)) for pose in P.SHEPPERD_POSES])


REFUSED = ("small/side", 9)  # by the rank test (tests/two_view_pose_ref.py); branch 0 at nine points is the case n9 above


def _family_id(case):
    pose, n, noise, kw = case
    return f"{pose}-n{n}" + ("-noise" if noise else "") + "".join(f"-{k}" for k in kw)


@pytest.mark.parametrize("case", FAMILY_CASES, ids=_family_id)
def test_bit_identity_on_the_pose_family(ftk, case):
    pose, n, noise, kw = case
    ref, cur, status = P.family_case(pose, n, noise)
    want = P.solve(ref, cur, status, **kw)
    assert int(want.valid[0]) == (-1 if (pose, n) == REFUSED else 1)
    assert P.same_results(_device(ftk, ref, cur, status, **kw), want) == [], case


def test_the_family_cases_reach_every_branch_of_the_quaternion_and_every_winner():
    """By the restatement's trace: a list pruned of a branch, of either outcome of the negation or of a winner fails here.  Each of the
    poses taken for a branch is on that branch at every size and in every call it is taken with."""
    traces = {_family_id(c): P.solve(*P.family_case(*c[:3]), **c[3]).trace for c in FAMILY_CASES}
    seen = np.array([t for t in traces.values() if t[P.TRACE_WINNER] >= 0])
    assert set(seen[:, P.TRACE_SHEPPERD]) == {0, 1, 2, 3} and set(seen[:, P.TRACE_NEGATED]) == {0, 1} and set(seen[:, P.TRACE_WINNER]) == {0, 1, 2, 3}
    for c in FAMILY_CASES:
        assert traces[_family_id(c)][P.TRACE_SHEPPERD] == (-1 if c[:2] == REFUSED else P.SHEPPERD_BRANCH[c[0].split("/")[0]]), c


@pytest.mark.parametrize("name", P.HOSTILE_CASES)
def test_hostile_and_degenerate_inputs(ftk, name):
    ref, cur, status = P.case(name)
    for threshold in (1.0, 0.0):
        want = P.solve(ref, cur, status, threshold=threshold)
        assert P.same_results(_device(ftk, ref, cur, status, threshold=threshold), want) == [], (name, threshold)


def test_a_second_camera_a_baseline_and_noise(ftk):
    ref, cur, _, _ = E.scene(300, 2, outlier_share=0.0, noise=0.3)
    status = np.full(300, P.TRACKED, np.uint8)
    for kw in (dict(K_cur=P.K_OTHER), dict(baseline=0.12), dict(threshold=0.5), dict(K=P.K_OTHER, K_cur=P.K, threshold=0.4, baseline=3.0)):
        want = P.solve(ref, cur, status, **kw)
        assert P.same_results(_device(ftk, ref, cur, status, **kw), want) == [], kw


def test_a_repeated_call_gives_equal_bits(ftk):
    ref, cur, status = P.case("n1025")
    solver = ftk.TwoViewPose(P.K)
    first, second = _device(ftk, ref, cur, status, solver), _device(ftk, ref, cur, status, solver)
    assert P.same_results(first, second) == [] and P.same_results(first, P.solve(ref, cur, status)) == []
    small = P.case("n9")  # the workspace of the larger call, left as it is
    assert P.same_results(_device(ftk, *small, solver), P.solve(*small)) == []


def test_a_captured_graph_replayed_on_changed_inputs_equals_the_eager_result(ftk):
    import torch
    ref, cur, _, _ = E.scene(300, 2, outlier_share=0.0, noise=0.3)
    ref2, cur2, _, _ = E.scene(300, 3, outlier_share=0.0)
    status = np.full(300, P.TRACKED, np.uint8)
    status2 = status.copy()
    status2[::5] = E.OUTSIDE
    solver = ftk.TwoViewPose(P.K, threshold=0.5)
    d_ref, d_cur, d_status = torch.from_numpy(ref.copy()).cuda(), torch.from_numpy(cur.copy()).cuda(), torch.from_numpy(status.copy()).cuda()
    solver.solve(d_ref, d_cur, d_status)  # the workspace is made here, outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = solver.solve(d_ref, d_cur, d_status)
    d_ref.copy_(torch.from_numpy(ref2))
    d_cur.copy_(torch.from_numpy(cur2))
    d_status.copy_(torch.from_numpy(status2))
    graph.replay()
    torch.cuda.synchronize()
    got = _host(d_status, out)
    assert P.same_results(got, _device(ftk, ref2, cur2, status2, threshold=0.5)) == []
    assert P.same_results(got, P.solve(ref2, cur2, status2, threshold=0.5)) == []


def test_filter_then_solve_equals_the_two_restatements_composed(ftk):
    """TwoViewRansac("fundamental").filter then TwoViewPose.solve on one scene with 30 % outliers, nothing read on the host in between."""
    import torch
    ref, cur, is_inlier, _ = E.scene(300, 1, noise=0.3)
    status = np.full(300, P.TRACKED, np.uint8)
    d_ref, d_cur, d_status = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda(), torch.from_numpy(status).cuda()
    fit = ftk.TwoViewRansac("fundamental", hypotheses=512, threshold=1.0, seed=1).filter(d_ref, d_cur, d_status, E.IMAGE)
    out = ftk.TwoViewPose(P.K, threshold=1.0).solve(d_ref, d_cur, d_status)
    torch.cuda.synchronize()
    filtered = T.ransac(ref, cur, status, E.IMAGE, 1.0, 512, 1, "fundamental")
    want = P.solve(ref, cur, filtered.status)
    assert int(fit.model.item()) == 0 and int(want.valid[0]) == 1 and int(want.n_points[0]) >= 150
    assert P.same_results(_host(d_status, out), want) == []


def test_filter_then_solve_on_a_half_turn_equals_the_two_restatements_composed(ftk):
    """The same composition at x170/side: the filter in front and the quaternion's x branch behind it, 30 % outliers, 0.3 px noise."""
    import torch
    ref, cur, _, _ = P.family_scene("x170/side", 300, 1, noise=0.3, outlier_share=0.3)
    status = np.full(300, P.TRACKED, np.uint8)
    d_ref, d_cur, d_status = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda(), torch.from_numpy(status).cuda()
    fit = ftk.TwoViewRansac("fundamental", hypotheses=512, threshold=1.0, seed=1).filter(d_ref, d_cur, d_status, E.IMAGE)
    out = ftk.TwoViewPose(P.K, threshold=1.0).solve(d_ref, d_cur, d_status)
    torch.cuda.synchronize()
    filtered = T.ransac(ref, cur, status, E.IMAGE, 1.0, 512, 1, "fundamental")
    want = P.solve(ref, cur, filtered.status)
    assert int(fit.model.item()) == 0 and int(want.valid[0]) == 1 and int(want.n_points[0]) >= 150 and want.trace[P.TRACE_SHEPPERD] == 1
    assert P.same_results(_host(d_status, out), want) == []


def test_the_context_stream_and_the_refusals_of_the_library(ftk):
    import torch
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    ref, cur, status = P.case("n257")
    ctx = D.context_on_stream(torch.cuda.Stream())
    got = _device(ftk, ref, cur, status, ftk.TwoViewPose(P.K, ctx=ctx))
    assert P.same_results(got, P.solve(ref, cur, status)) == []
    t = torch.zeros(16, 2, device="cuda")
    st = torch.ones(16, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(1000, dtype=torch.int64, device="cuda")
    o = torch.zeros(16, dtype=torch.int32, device="cuda")
    f = torch.zeros(64, device="cuda")
    call = lambda n=16, fx=500.0, cx=320.0, fy_cur=500.0, threshold=1.0, baseline=1.0: N.lib().ftk_two_view_pose_device(  # noqa: E731
        ctx.handle, None, t.data_ptr(), t.data_ptr(), st.data_ptr(), n, fx, 500.0, cx, 240.0, 500.0, fy_cur, 320.0, 240.0, threshold, baseline, ws.data_ptr(),
        f.data_ptr(), f.data_ptr(), f.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr())
    inf, nan = float("inf"), float("nan")
    assert call(n=N.FTK_TRACK_TABLE_MAX_SLOTS + 1) == -4 and call(n=0) == -1  # FTK_E_UNSUPPORTED, FTK_E_INVALID_ARGUMENT: nothing launched
    assert call(fx=0.0) == -1 and call(fx=-1.0) == -1 and call(fx=nan) == -1 and call(fx=inf) == -1 and call(fy_cur=0.0) == -1 and call(cx=nan) == -1
    assert call(threshold=-1.0) == -1 and call(threshold=nan) == -1 and call(threshold=inf) == -1 and call(threshold=2.0e19) == -1 and call(fx=1e-50) == -1
    assert call(baseline=0.0) == -1 and call(baseline=-0.5) == -1 and call(baseline=nan) == -1 and call(baseline=inf) == -1
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == [1] * 16 and not f.any() and not o.any()
