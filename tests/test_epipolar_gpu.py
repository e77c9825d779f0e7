"""EpipolarRansac on the device against the scalar restatement (tests/epipolar_ref.c): status, best, n_inliers, F, counts and
models bit for bit, at the sizes that cross the scan's and the scoring tile's edges, on hostile and degenerate inputs, repeated, and replayed
from a captured graph."""
import numpy as np
import pytest

from tests import epipolar_ref as E

pytestmark = pytest.mark.gpu

FIELDS = ("status", "F", "counts", "models")


def _device(ftk, ref, cur, status, image, threshold, K, seed, ransac=None):
    import torch
    d_ref, d_cur, d_status = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda(), torch.from_numpy(status).cuda()
    ransac = ransac or ftk.EpipolarRansac(hypotheses=K, threshold=threshold, seed=seed)
    out = ransac.filter(d_ref, d_cur, d_status, image, return_hypotheses=True)
    torch.cuda.synchronize()
    assert E.same(d_ref.cpu().numpy(), ref) and E.same(d_cur.cpu().numpy(), cur)  # inputs other than status are untouched
    return dict(status=d_status.cpu().numpy(), F=out.F.cpu().numpy(), counts=out.counts.cpu().numpy(), models=out.models.cpu().numpy(),
                best=int(out.best.item()), n_inliers=int(out.n_inliers.item()))


def _equal(got, want, what):
    for field in FIELDS:
        assert E.same(got[field], getattr(want, field)), (what, field)
    assert (got["best"], got["n_inliers"]) == (want.best, want.n_inliers), what


@pytest.mark.parametrize("K", [1, 63, 65, 1000])
@pytest.mark.parametrize("name", ["n7", "n8", "n9", "n64_half", "n257", "n1025"])
def test_bit_identity_with_the_restatement(ftk, name, K):
    ref, cur, status, image = E.case(name)
    want = E.ransac(ref, cur, status, image, 1.0, K, 3)
    _equal(_device(ftk, ref, cur, status, image, 1.0, K, 3), want, (name, K))


def test_a_winner_beyond_the_first_hypothesis_of_every_select_thread(ftk):
    """2048 hypotheses: a thread of the select kernel folds two.  The 300-point scene with 0.3 px of noise (without noise the first sample
    of inliers alone wins, an early one); under this seed the winner (best = 1543) is a thread's second."""
    ref, cur, _, _ = E.scene(300, 1, noise=0.3)
    status = np.full(300, E.TRACKED, np.uint8)
    want = E.ransac(ref, cur, status, E.IMAGE, 1.0, 2048, 4)
    assert want.best >= 1024
    _equal(_device(ftk, ref, cur, status, E.IMAGE, 1.0, 2048, 4), want, "fold")


@pytest.mark.parametrize("name", E.HOSTILE_CASES)
def test_hostile_and_degenerate_inputs(ftk, name):
    ref, cur, status, image = E.case(name)
    for threshold in (1.0, 0.0):
        want = E.ransac(ref, cur, status, image, threshold, 64, 0)
        _equal(_device(ftk, ref, cur, status, image, threshold, 64, 0), want, (name, threshold))


def test_a_scene_is_cleaned_and_a_repeated_call_gives_equal_bits(ftk):
    ref, cur, is_inlier, _ = E.scene(300, 1)
    status = np.full(300, E.TRACKED, np.uint8)
    ransac = ftk.EpipolarRansac(hypotheses=512, threshold=1.0, seed=1)
    first = _device(ftk, ref, cur, status, E.IMAGE, 1.0, 512, 1, ransac)
    second = _device(ftk, ref, cur, status, E.IMAGE, 1.0, 512, 1, ransac)
    _equal(first, E.ransac(ref, cur, status, E.IMAGE, 1.0, 512, 1), "scene")
    for field in FIELDS + ("best", "n_inliers"):
        assert E.same(first[field], second[field]) if field in FIELDS else first[field] == second[field], field
    assert np.array_equal(first["status"] == E.TRACKED, is_inlier)


def test_a_captured_graph_replayed_on_changed_inputs_equals_the_eager_result(ftk):
    import torch
    ref, cur, _, _ = E.scene(300, 2)
    ref2, cur2, _, _ = E.scene(300, 3)
    status = np.full(300, E.TRACKED, np.uint8)
    status2 = status.copy()
    status2[::5] = E.OUTSIDE
    ransac = ftk.EpipolarRansac(hypotheses=65, threshold=1.0, seed=9)
    d_ref, d_cur, d_status = torch.from_numpy(ref.copy()).cuda(), torch.from_numpy(cur.copy()).cuda(), torch.from_numpy(status.copy()).cuda()
    ransac.filter(d_ref, d_cur, d_status, E.IMAGE)  # the workspace is made here, outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ransac.filter(d_ref, d_cur, d_status, E.IMAGE, return_hypotheses=True)
    d_ref.copy_(torch.from_numpy(ref2))
    d_cur.copy_(torch.from_numpy(cur2))
    d_status.copy_(torch.from_numpy(status2))
    graph.replay()
    torch.cuda.synchronize()
    got = dict(status=d_status.cpu().numpy(), F=out.F.cpu().numpy(), counts=out.counts.cpu().numpy(), models=out.models.cpu().numpy(),
               best=int(out.best.item()), n_inliers=int(out.n_inliers.item()))
    eager = _device(ftk, ref2, cur2, status2, E.IMAGE, 1.0, 65, 9)
    for field in FIELDS + ("best", "n_inliers"):
        assert E.same(got[field], eager[field]) if field in FIELDS else got[field] == eager[field], field
    _equal(got, E.ransac(ref2, cur2, status2, E.IMAGE, 1.0, 65, 9), "replay")


def test_the_context_stream_and_the_refusals_of_the_library(ftk):
    import torch
    from feature_tracker_amd import device as D
    ref, cur, status, image = E.case("n257")
    ctx = D.context_on_stream(torch.cuda.Stream())
    got = _device(ftk, ref, cur, status, image, 1.0, 63, 3, ftk.EpipolarRansac(63, 1.0, 3, ctx=ctx))
    _equal(got, E.ransac(ref, cur, status, image, 1.0, 63, 3), "context stream")
    from feature_tracker_amd import _native as N
    t = torch.zeros(16, 2, device="cuda")
    st = torch.ones(16, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(100000, dtype=torch.int64, device="cuda")
    o = torch.zeros(16, dtype=torch.int32, device="cuda")
    F = torch.zeros(3, 3, device="cuda")
    call = lambda n, k, rows=480: N.lib().ftk_epipolar_ransac_device(ctx.handle, None, t.data_ptr(), t.data_ptr(), st.data_ptr(), n, rows, 640, 1.0, k, 0,  # noqa: E731
                                                                     ws.data_ptr(), o.data_ptr(), o.data_ptr(), F.data_ptr(), None, None)
    assert call(16, N.FTK_EPIPOLAR_MAX_HYPOTHESES + 1) == -4 and call(N.FTK_TRACK_TABLE_MAX_SLOTS + 1, 8) == -4  # FTK_E_UNSUPPORTED, nothing launched
    assert call(0, 8) == -1 and call(16, 0) == -1 and call(16, 8, rows=0) == -1
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == [1] * 16


def test_bit_identity_on_the_pose_family(ftk):
    """A pose per branch of TwoViewPose's quaternion and forward motion (tests/two_view_pose_ref.py), 30 % outliers."""
    from tests import two_view_pose_ref as P
    for pose in P.FILTER_POSES:
        ref, cur, _, _ = P.family_scene(pose, 300, 1, outlier_share=0.3)
        status = np.full(300, E.TRACKED, np.uint8)
        _equal(_device(ftk, ref, cur, status, E.IMAGE, 1.0, 512, 1), E.ransac(ref, cur, status, E.IMAGE, 1.0, 512, 1), pose)
