"""MatchAssignment on the device against the scalar restatement (tests/match_assignment_ref.c): every entry of ``scores``
bit for bit, any NaN equal to any NaN."""
import numpy as np
import pytest

from tests import match_assignment_ref as R

pytestmark = pytest.mark.gpu

IDS = ["x".join(str(v) for v in s[:3]) for s in R.SHAPES]
FORMS = pytest.mark.parametrize("with_weights", [False, True], ids=["without_weights", "with_weights"])


def _head(ftk, shape, with_weights, ctx=None):
    import torch
    if not with_weights:
        return ftk.MatchAssignment.without_weights(shape[2], ctx=ctx)
    fw, fb, mw, mb = (torch.from_numpy(x.copy()) for x in R.head_weights(shape[2], shape[3] + 1000))
    sd = {"log_assignment.8.final_proj.weight": fw, "log_assignment.8.final_proj.bias": fb, "log_assignment.8.matchability.weight": mw,
          "log_assignment.8.matchability.bias": mb}
    return ftk.MatchAssignment.from_state_dict(sd, ctx=ctx)


def _count(c):
    import torch
    return None if c is None else torch.tensor([c], dtype=torch.int32, device="cuda")


def _device(head, a, b, count0=None, count1=None, row_stride=None):
    """scores on the host; the inputs must come back untouched."""
    import torch
    d_a, d_b = torch.from_numpy(np.array(a, copy=True)).cuda(), torch.from_numpy(np.array(b, copy=True)).cuda()
    scores = head.assign(d_a, d_b, _count(count0), _count(count1), row_stride=row_stride)
    torch.cuda.synchronize()
    assert R.same(d_a.cpu().numpy(), a) and R.same(d_b.cpu().numpy(), b)
    assert tuple(scores.shape) == (a.shape[0] + 1, b.shape[0] + 1)
    return scores.cpu().numpy()


@FORMS
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_bit_identity_with_the_restatement(ftk, shape, with_weights):
    a, b, kw = R.case(shape, with_weights)
    assert R.same(_device(_head(ftk, shape, with_weights), a, b), R.assign(a, b, **kw))


@FORMS
def test_counts_on_the_device(ftk, with_weights):
    shape = R.SHAPES[7]
    a, b, kw = R.case(shape, with_weights)
    m, n = shape[:2]
    head = _head(ftk, shape, with_weights)
    for c0, c1 in ((0, None), (None, 0), (1, 1), (65, 64), (33, 77), (m, n), (m + 5, n + 1000), (-4, 3), (0, 0)):
        assert R.same(_device(head, a, b, c0, c1), R.assign(a, b, count0=c0, count1=c1, **kw)), (c0, c1)


@FORMS
def test_a_padded_row_stride_leaves_the_padding(ftk, with_weights):
    import torch
    shape = R.SHAPES[9]
    a, b, kw = R.case(shape, with_weights)
    m, n = shape[:2]
    head = _head(ftk, shape, with_weights)
    want = R.assign(a, b, **kw)
    stride = 136  # rows 16-byte aligned
    assert R.same(_device(head, a, b, row_stride=stride), want)
    buf = torch.full((m + 1, stride), float(R.SENTINEL), device="cuda")
    out = buf[:, :n + 1]
    got = head.assign(torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda(), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and R.same(got.cpu().numpy(), want)
    assert (buf[:, n + 1:].cpu().numpy() == R.SENTINEL).all()


@FORMS
@pytest.mark.parametrize("index", [4, 5, 7])
def test_hostile_descriptors(ftk, index, with_weights):
    shape = R.SHAPES[index]
    a, b = R.hostile(shape)
    _, _, kw = R.case(shape, with_weights)
    want = R.assign(a, b, **kw)
    assert np.isnan(want).any() and np.isfinite(want).any()
    assert R.same(_device(_head(ftk, shape, with_weights), a, b), want)
    assert R.same(_device(_head(ftk, shape, with_weights), a, b, 20, 40), R.assign(a, b, count0=20, count1=40, **kw))


@FORMS
def test_a_repeated_call_gives_the_same_bits(ftk, with_weights):
    shape, other = R.SHAPES[7], R.SHAPES[6]
    a, b, kw = R.case(shape, with_weights)
    head = _head(ftk, shape, with_weights)
    first = _device(head, a, b)
    a2, b2, _ = R.case(other, with_weights)  # another size in between: its own workspace
    _device(head, a2, b2)
    second = _device(head, a, b)
    assert R.same(first, second) and R.same(first, R.assign(a, b, **kw))


@FORMS
def test_a_captured_graph_replayed_on_changed_descriptors_and_counts_equals_the_eager_call(ftk, with_weights):
    import torch
    shape = R.SHAPES[7]
    a, b, kw = R.case(shape, with_weights)
    m, n, d, seed = shape
    a2, b2 = R.descriptors(m, n, d, seed + 50)
    head = _head(ftk, shape, with_weights)
    d_a, d_b = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    c0, c1 = _count(m), _count(n)
    head.match(d_a, d_b, c0, c1, min_score=-20.0)  # the workspaces are made here, outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scores, index, status = head.match(d_a, d_b, c0, c1, min_score=-20.0)
    d_a.copy_(torch.from_numpy(a2))
    d_b.copy_(torch.from_numpy(b2))
    c0.fill_(70)
    c1.fill_(101)
    graph.replay()
    torch.cuda.synchronize()
    want = R.assign(a2, b2, count0=70, count1=101, **kw)
    assert R.same(scores.cpu().numpy(), want) and R.same(scores.cpu().numpy(), _device(head, a2, b2, 70, 101))
    from tests import nn_match_ref
    want_index, want_status = nn_match_ref.match_scores(want[:m, :n], -20.0)
    assert np.array_equal(index.cpu().numpy(), want_index) and np.array_equal(status.cpu().numpy(), want_status)
    assert (want_index[:70] >= 0).sum() >= 40 and (want_index[70:] == -1).all()


def test_the_context_stream_and_the_refusals_of_the_library(ftk):
    import torch
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    shape = R.SHAPES[5]
    a, b, kw = R.case(shape, True)
    ctx = D.context_on_stream(torch.cuda.Stream())
    assert R.same(_device(_head(ftk, shape, True, ctx=ctx), a, b), R.assign(a, b, **kw))
    x, y = torch.zeros(4, 8, device="cuda"), torch.zeros(5, 8, device="cuda")
    ws = torch.zeros(4096, dtype=torch.int64, device="cuda")
    out = torch.full((5 * 6,), 7.0, device="cuda")
    call = lambda m=4, n=5, d=8, scale=0.5, stride=0: N.lib().ftk_match_assignment_device(  # noqa: E731
        ctx.handle, None, x.data_ptr(), m, y.data_ptr(), n, d, None, None, scale, None, None, ws.data_ptr(), out.data_ptr(), stride)
    assert call(m=0) == -1 and call(n=4097) == -1 and call(d=0) == -1 and call(d=1025) == -1 and call(stride=5) == -1
    assert call(scale=0.0) == -1 and call(scale=float("nan")) == -1 and call(scale=float("inf")) == -1 and call(scale=-1.0) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()  # nothing was launched
    assert call() == 0


def test_heads_to_assignment_to_the_two_view_filter_without_a_host_read(ftk):
    """Two head pairs of one scene shifted by a whole number of cells: KeypointDecoder on both, MatchAssignment.without_weights(...).match
    with the decoder's count tensors, TwoViewRansac with a homography, all on one stream.  Nothing is read on the host before the final
    comparison, which is against the restatements composed."""
    import torch
    from feature_tracker_amd import device as D
    from tests import keypoint_decode_ref as K
    from tests import nn_match_ref
    from tests import two_view_ref as T
    k, shift = 300, (1, 2)  # cells down, cells right
    semi, desc = K.heads(9, 17, 64, 41)
    semi2, desc2 = np.roll(semi, shift, axis=(1, 2)), np.roll(desc, shift, axis=(1, 2))
    kw = dict(min_score=0.05, min_distance=6, border=4)
    scale, min_score = 3.0, -20.0
    stream = torch.cuda.Stream()
    ctx = D.context_on_stream(stream)
    with torch.cuda.stream(stream):
        decoder = ftk.KeypointDecoder(max_keypoints=k, ctx=ctx, **kw)
        a = decoder.decode(torch.from_numpy(semi.copy()).cuda(), torch.from_numpy(desc.copy()).cuda())
        b = decoder.decode(torch.from_numpy(semi2.copy()).cuda(), torch.from_numpy(desc2.copy()).cuda())
        head = ftk.MatchAssignment.without_weights(64, scale=scale, ctx=ctx)
        scores, index, status = head.match(a.descriptors, b.descriptors, a.count, b.count, min_score=min_score)
        cur_uv = b.uv[index.clamp(min=0).long()]
        before = status.clone()
        fit = ftk.TwoViewRansac(model="homography", hypotheses=64, threshold=1.0, seed=2, ctx=ctx).filter(a.uv, cur_uv, status, (72, 136))
    stream.synchronize()
    # ---- the final comparison ----
    want_a, want_b = K.decode(semi, desc, max_keypoints=k, **kw), K.decode(semi2, desc2, max_keypoints=k, **kw)
    assert 10 <= want_a.count < k and 10 <= want_b.count < k
    want_scores = R.assign(want_a.descriptors, want_b.descriptors, scale=scale, count0=want_a.count, count1=want_b.count)
    assert R.same(scores.cpu().numpy(), want_scores)
    want_index, want_status = nn_match_ref.match_scores(want_scores[:k, :k], min_score)
    got_index = index.cpu().numpy()
    assert np.array_equal(got_index, want_index) and np.array_equal(before.cpu().numpy(), want_status)
    assert (got_index[want_a.count:] == -1).all() and (got_index < want_b.count).all()
    matched = got_index >= 0
    moved = want_b.uv[got_index[matched]] - want_a.uv[matched]
    assert (moved == np.float32([16.0, 8.0])).all(axis=1).sum() >= 10
    want_fit = T.ransac(want_a.uv, want_b.uv[np.clip(want_index, 0, None)], want_status, (72, 136), 1.0, 64, 2, "homography")
    assert np.array_equal(status.cpu().numpy(), want_fit.status) and int(fit.model.item()) == want_fit.model == 1
    assert int((status == 1).sum().item()) >= 10
