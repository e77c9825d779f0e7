"""TwoViewRansac on the device against the scalar restatement (tests/two_view_ref.c): model, status, best, n_inliers, F, H,
counts and models bit for bit in all three modes, at the sizes that cross the samplers', the scan's and the scoring tile's edges, on hostile
and degenerate inputs, against EpipolarRansac on the device, repeated, and replayed from a captured graph."""
import numpy as np
import pytest

from tests import epipolar_ref as E
from tests import two_view_ref as T

pytestmark = pytest.mark.gpu

MODES = ("fundamental", "homography", "auto")


def _device(ftk, ref, cur, status, image, threshold, K, seed, mode, ransac=None, permille=750):
    import torch
    d_ref, d_cur, d_status = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda(), torch.from_numpy(status).cuda()
    ransac = ransac or ftk.TwoViewRansac(model=mode, hypotheses=K, threshold=threshold, prefer_homography=permille / 1000.0, seed=seed)
    out = ransac.filter(d_ref, d_cur, d_status, image, return_hypotheses=True)
    torch.cuda.synchronize()
    assert E.same(d_ref.cpu().numpy(), ref) and E.same(d_cur.cpu().numpy(), cur)  # inputs other than status are untouched
    return _host(d_status, out)


def _host(d_status, out):
    r = T.Result()
    r.status, r.model = d_status.cpu().numpy(), int(out.model.item())
    for name in ("best", "n_inliers", "F", "H", "counts", "models"):
        setattr(r, name, getattr(out, name).cpu().numpy())
    return r


@pytest.mark.parametrize("K", [1, 63, 65, 1000])
@pytest.mark.parametrize("name", ["n3", "n4", "n5", "n7", "n8", "n9", "n64_half", "n257", "n1025", "plane300"])
def test_bit_identity_with_the_restatement(ftk, name, K):
    ref, cur, status, image = T.case(name)
    for mode in MODES:
        want = T.ransac(ref, cur, status, image, 1.0, K, 3, mode)
        assert T.same_results(_device(ftk, ref, cur, status, image, 1.0, K, 3, mode), want) == [], (name, K, mode)


def test_winners_beyond_the_first_hypothesis_of_every_select_thread(ftk):
    """2048 hypotheses: a thread of the select kernel folds two of each model.  The 300-point scene with 0.3 px of noise (without noise
    the first sample of inliers alone wins, an early one); under this seed both winners (best = 1543, 1664) are a thread's second."""
    ref, cur, _, _ = E.scene(300, 1, noise=0.3)
    status = np.full(300, T.TRACKED, np.uint8)
    for mode in MODES:
        want = T.ransac(ref, cur, status, T.IMAGE, 1.0, 2048, 4, mode)
        assert min(b for b in want.best if b >= 0) >= 1024
        assert T.same_results(_device(ftk, ref, cur, status, T.IMAGE, 1.0, 2048, 4, mode), want) == [], mode


@pytest.mark.parametrize("name", T.HOSTILE_CASES)
def test_hostile_and_degenerate_inputs(ftk, name):
    ref, cur, status, image = T.case(name)
    for mode in MODES:
        for threshold in (1.0, 0.0):
            want = T.ransac(ref, cur, status, image, threshold, 64, 0, mode)
            assert T.same_results(_device(ftk, ref, cur, status, image, threshold, 64, 0, mode), want) == [], (name, mode, threshold)


def test_the_preference_and_its_bounds(ftk):
    ref, cur, status, image = T.case("plane300")
    for permille in (0, 850, 1000):
        want = T.ransac(ref, cur, status, image, 1.0, 65, 5, "auto", permille)
        assert T.same_results(_device(ftk, ref, cur, status, image, 1.0, 65, 5, "auto", permille=permille), want) == [], permille


def test_mode_fundamental_equals_epipolar_ransac_on_the_device(ftk):
    import torch
    for name, K in (("n9", 63), ("n257", 65), ("n1025", 1000), ("hostile", 64)):
        ref, cur, status, image = T.case(name)
        got = _device(ftk, ref, cur, status, image, 1.0, K, 3, "fundamental")
        d_ref, d_cur, d_status = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda(), torch.from_numpy(status).cuda()
        out = ftk.EpipolarRansac(hypotheses=K, threshold=1.0, seed=3).filter(d_ref, d_cur, d_status, image, return_hypotheses=True)
        torch.cuda.synchronize()
        assert E.same(got.status, d_status.cpu().numpy()) and E.same(got.F, out.F.cpu().numpy()), name
        assert E.same(got.counts[0], out.counts.cpu().numpy()) and E.same(got.models[0], out.models.cpu().numpy()), name
        assert (int(got.best[0]), int(got.n_inliers[0])) == (int(out.best.item()), int(out.n_inliers.item())), name
        assert got.model == (0 if got.best[0] >= 0 else -1) and got.best[1] == -1 and not got.H.any() and (got.counts[1] == -1).all()


def test_a_planar_scene_is_cleaned_and_a_repeated_call_gives_equal_bits(ftk):
    ref, cur, on_patch, _ = T.planar_scene(300, 1, "moving", 0.0)
    status = np.full(300, T.TRACKED, np.uint8)
    ransac = ftk.TwoViewRansac(hypotheses=512, threshold=1.0, seed=1)
    first = _device(ftk, ref, cur, status, T.IMAGE, 1.0, 512, 1, "auto", ransac)
    second = _device(ftk, ref, cur, status, T.IMAGE, 1.0, 512, 1, "auto", ransac)
    assert T.same_results(first, T.ransac(ref, cur, status, T.IMAGE, 1.0, 512, 1, "auto")) == [] and T.same_results(first, second) == []
    assert first.model == 1 and np.array_equal(first.status == T.LARGE_RESIDUAL, on_patch)


def test_a_captured_graph_replayed_on_changed_inputs_equals_the_eager_result(ftk):
    import torch
    ref, cur, _, _ = T.planar_scene(300, 2, "moving", 0.3)
    ref2, cur2, _, _ = E.scene(300, 3)
    status = np.full(300, T.TRACKED, np.uint8)
    status2 = status.copy()
    status2[::5] = E.OUTSIDE
    for mode in MODES:
        ransac = ftk.TwoViewRansac(model=mode, hypotheses=65, threshold=1.0, seed=9)
        d_ref, d_cur, d_status = torch.from_numpy(ref.copy()).cuda(), torch.from_numpy(cur.copy()).cuda(), torch.from_numpy(status.copy()).cuda()
        ransac.filter(d_ref, d_cur, d_status, T.IMAGE)  # the workspace is made here, outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ransac.filter(d_ref, d_cur, d_status, T.IMAGE, return_hypotheses=True)
        d_ref.copy_(torch.from_numpy(ref2))
        d_cur.copy_(torch.from_numpy(cur2))
        d_status.copy_(torch.from_numpy(status2))
        graph.replay()
        torch.cuda.synchronize()
        got = _host(d_status, out)
        assert T.same_results(got, _device(ftk, ref2, cur2, status2, T.IMAGE, 1.0, 65, 9, mode)) == [], mode
        assert T.same_results(got, T.ransac(ref2, cur2, status2, T.IMAGE, 1.0, 65, 9, mode)) == [], mode


def test_the_context_stream_and_the_refusals_of_the_library(ftk):
    import torch
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    ref, cur, status, image = T.case("n257")
    ctx = D.context_on_stream(torch.cuda.Stream())
    got = _device(ftk, ref, cur, status, image, 1.0, 63, 3, "auto", ftk.TwoViewRansac("auto", 63, 1.0, 0.75, 3, ctx=ctx))
    assert T.same_results(got, T.ransac(ref, cur, status, image, 1.0, 63, 3, "auto")) == []
    t = torch.zeros(16, 2, device="cuda")
    st = torch.ones(16, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(100000, dtype=torch.int64, device="cuda")
    o = torch.zeros(16, dtype=torch.int32, device="cuda")
    M = torch.zeros(3, 3, device="cuda")
    call = lambda n, k, mode=2, p=750, rows=480: N.lib().ftk_two_view_ransac_device(  # noqa: E731
        ctx.handle, None, t.data_ptr(), t.data_ptr(), st.data_ptr(), n, rows, 640, 1.0, k, 0, mode, p, ws.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(),
        M.data_ptr(), M.data_ptr(), None, None)
    assert call(16, N.FTK_EPIPOLAR_MAX_HYPOTHESES + 1) == -4 and call(N.FTK_TRACK_TABLE_MAX_SLOTS + 1, 8) == -4  # FTK_E_UNSUPPORTED, nothing launched
    assert call(0, 8) == -1 and call(16, 0) == -1 and call(16, 8, rows=0) == -1
    assert call(16, 8, mode=3) == -1 and call(16, 8, mode=-1) == -1 and call(16, 8, p=1001) == -1 and call(16, 8, p=-1) == -1
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == [1] * 16


def test_bit_identity_on_the_pose_family(ftk):
    """A pose per branch of TwoViewPose's quaternion and forward motion (tests/two_view_pose_ref.py): the fundamental
    matrix on the depth scene with 30 % outliers, the homography on the plane with its patch."""
    from tests import two_view_pose_ref as P
    status = np.full(300, T.TRACKED, np.uint8)
    for pose in P.FILTER_POSES:
        ref, cur, _, _ = P.family_scene(pose, 300, 1, outlier_share=0.3)
        want = T.ransac(ref, cur, status, T.IMAGE, 1.0, 512, 1, "fundamental")
        assert T.same_results(_device(ftk, ref, cur, status, T.IMAGE, 1.0, 512, 1, "fundamental"), want) == [], pose
        ref, cur, _, _ = T.planar_scene(300, 1, "moving", 0.0, pose=P.family_pose(pose))
        want = T.ransac(ref, cur, status, T.IMAGE, 1.0, 512, 1, "homography")
        assert T.same_results(_device(ftk, ref, cur, status, T.IMAGE, 1.0, 512, 1, "homography"), want) == [], pose
