"""PnpRansac(sample="p3p") on the device against the scalar restatement (tests/pnp_p3p_ref.c): pose, n_inliers, best, valid,
status, counts and models bit for bit at every edge of the participant count (3: invalid; 4 and 5: no refit step; 6, 7; the 256-point
tiles; 65 536 points), at hypothesis counts that cross the one-lane-per-hypothesis workgroup, on the hostile, degenerate and planar
cases, with and without the refit, with unequal focal lengths, and replayed from a captured graph."""
import numpy as np
import pytest

from tests import epipolar_ref as E
from tests import pnp_p3p_ref as Q
from tests import pnp_ref as R

pytestmark = pytest.mark.gpu

ALL = R.OUTPUTS + R.HYPOTHESES


def _host(d_status, out, hypotheses=True):
    r = R.Result()
    r.status = d_status.cpu().numpy()
    for name in ("pose", "n_inliers", "best", "valid") + (R.HYPOTHESES if hypotheses else ()):
        setattr(r, name, getattr(out, name).cpu().numpy())
    return r


def _device(ftk, X, uv, status, solver=None, seed=None, return_hypotheses=True, **kw):
    import torch
    d_X, d_uv, d_status = torch.from_numpy(X).cuda(), torch.from_numpy(uv).cuda(), torch.from_numpy(status).cuda()
    solver = solver or ftk.PnpRansac(kw.pop("K", R.K), sample="p3p", **kw)
    out = solver.solve(d_X, d_uv, d_status, seed=seed, return_hypotheses=return_hypotheses)
    torch.cuda.synchronize()
    assert E.same(d_X.cpu().numpy(), X) and E.same(d_uv.cpu().numpy(), uv)
    return _host(d_status, out, return_hypotheses)


@pytest.mark.parametrize("name", Q.SIZE_CASES)
def test_bit_identity_at_every_edge_of_the_participant_count(ftk, name):
    X, uv, status = Q.case(name)
    want = Q.solve(X, uv, status)
    assert int(want.valid[0]) == (-1 if name == "n3" else 1)
    if name in ("n4", "n5"):
        assert want.trace[R.TRACE_STEP0] == R.STEP_FEW_INLIERS and want.trace[R.TRACE_STEPS] == 0  # the pose is the winner's
    assert R.same_results(_device(ftk, X, uv, status), want, ALL) == [], name


@pytest.mark.parametrize("hypotheses", [1, 63, 64, 65, 512, 4096])
def test_hypothesis_counts_across_the_workgroup(ftk, hypotheses):
    X, uv, status = Q.case("n64")
    want = Q.solve(X, uv, status, hypotheses=hypotheses, seed=5)
    assert R.same_results(_device(ftk, X, uv, status, hypotheses=hypotheses, seed=5), want, ALL) == [], hypotheses


def test_a_winner_beyond_the_first_hypothesis_of_every_select_thread(ftk):
    """2048 hypotheses: a thread of the select kernel folds two, and under this seed the winner (best = 1950) is a thread's second."""
    X, uv, _, _ = R.scene(300, 2, noise=0.3, outlier_share=0.3)
    status = np.full(300, R.TRACKED, np.uint8)
    want = Q.solve(X, uv, status, hypotheses=2048, seed=0)
    assert int(want.valid[0]) == 1 and int(want.best[0]) >= 1024
    assert R.same_results(_device(ftk, X, uv, status, hypotheses=2048, seed=0), want, ALL) == []


@pytest.mark.parametrize("name", Q.NAMED_CASES)
def test_hostile_degenerate_and_planar_inputs(ftk, name):
    X, uv, status = Q.case(name)
    for threshold in (1.0, 0.0):
        want = Q.solve(X, uv, status, threshold=threshold)
        assert R.same_results(_device(ftk, X, uv, status, threshold=threshold), want, ALL) == [], (name, threshold)
    if name == "coplanar":
        X, uv, status = Q.case(name)
        got = _device(ftk, X, uv, status)
        assert int(got.valid[0]) == 1 and int(got.n_inliers[0]) == 40  # the capability: no setting of "dlt6" gives a pose here


def test_the_tilted_plane_with_outliers(ftk):
    X, uv, is_inlier, _ = Q.tilted_plane()
    status = np.full(len(X), R.TRACKED, np.uint8)
    got = _device(ftk, X, uv, status)
    assert R.same_results(got, Q.solve(X, uv, status), ALL) == []
    assert int(got.valid[0]) == 1 and np.array_equal(got.status == R.TRACKED, is_inlier)


def test_a_wide_view_and_unequal_focal_lengths(ftk):
    X, uv, status, _ = R.wide_case()
    assert R.same_results(_device(ftk, X, uv, status, K=R.K_WIDE), Q.solve(X, uv, status, K=R.K_WIDE), ALL) == []
    X, uv, _, _ = R.family_scene("small/side", 300, 1, 0.3, 0.3, R.K_OTHER)
    status = np.full(300, R.TRACKED, np.uint8)
    want = Q.solve(X, uv, status, K=R.K_OTHER, threshold=0.5)
    assert int(want.valid[0]) == 1 and R.same_results(_device(ftk, X, uv, status, K=R.K_OTHER, threshold=0.5), want, ALL) == []


@pytest.mark.parametrize("refine", [0, 4])
def test_with_and_without_the_refit(ftk, refine):
    X, uv, _, _ = R.scene(300, 3, noise=0.3, outlier_share=0.3)
    status = np.full(300, R.TRACKED, np.uint8)
    want = Q.solve(X, uv, status, refine_iterations=refine, seed=2)
    assert int(want.valid[0]) == 1 and want.trace[R.TRACE_STEPS] == refine
    assert R.same_results(_device(ftk, X, uv, status, refine_iterations=refine, seed=2), want, ALL) == [], refine


def test_two_seeds_and_a_call_without_the_hypotheses(ftk):
    X, uv, _, _ = R.scene(300, 2, noise=0.3, outlier_share=0.3)
    status = np.full(300, R.TRACKED, np.uint8)
    a, b = _device(ftk, X, uv, status, seed=4), _device(ftk, X, uv, status, seed=5)
    assert int(a.best[0]) != int(b.best[0]) and R.same_results(a, Q.solve(X, uv, status, seed=4), ALL) == []
    assert R.same_results(_device(ftk, X, uv, status, seed=4, return_hypotheses=False), a, R.OUTPUTS) == []


def test_dlt6_by_name_is_the_call_without_a_sampler(ftk):
    import torch
    X, uv, status = R.case("n257")
    d = [torch.from_numpy(a).cuda() for a in (X, uv, status)]
    out = ftk.PnpRansac(R.K, sample="dlt6").solve(*d, return_hypotheses=True)
    torch.cuda.synchronize()
    assert R.same_results(_host(d[2], out), R.solve(X, uv, status), ALL) == []


def test_a_captured_graph_replayed_equals_the_eager_call(ftk):
    import torch
    X, uv, _, _ = R.scene(300, 2, noise=0.3, outlier_share=0.3)
    status = np.full(300, R.TRACKED, np.uint8)
    solver = ftk.PnpRansac(R.K, threshold=0.5, seed=9, sample="p3p")
    eager = _device(ftk, X, uv, status, solver)  # the workspace is made here, outside the capture
    d_X, d_uv, d_status = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(uv.copy()).cuda(), torch.from_numpy(status.copy()).cuda()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = solver.solve(d_X, d_uv, d_status, return_hypotheses=True)
    d_status.copy_(torch.from_numpy(status))
    graph.replay()
    torch.cuda.synchronize()
    got = _host(d_status, out)
    assert R.same_results(got, eager, ALL) == [] and R.same_results(got, Q.solve(X, uv, status, threshold=0.5, seed=9), ALL) == []
