"""``LightGlue.match_adaptive`` and ``device.lightglue_confidence_device`` on the device against the scalar restatement
(tests/lightglue_adaptive_ref.c): every specified output bit for bit.  L = 3 and pruning_min_keypoints = 0 unless said
otherwise.  The rotary encoding is an input of the contract (tests/test_transformer_gpu.py): the restatement takes the device's."""
import functools

import numpy as np
import pytest

from tests import lightglue_adaptive_ref as R
from tests import transformer_ref as T

pytestmark = pytest.mark.gpu

IDS = ["x".join(str(v) for v in s[:4]) for s in R.SHAPES]
PRUNING_SHAPES = R.SHAPES[1:]


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def _count(c):
    import torch
    return None if c is None else torch.tensor([c], dtype=torch.int32, device="cuda")


def _lightglue(ftk, sd, heads, depth, width, min_keypoints=0, ctx=None):
    import torch
    return ftk.LightGlue.from_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, num_heads=heads, ctx=ctx, depth_confidence=depth,
                                         width_confidence=width, pruning_min_keypoints=min_keypoints)


def _host(result):
    """A device result as the restatement's namespace."""
    import torch
    from types import SimpleNamespace
    torch.cuda.synchronize()
    f = {k: getattr(result, k).cpu().numpy() for k in result.__slots__}
    return SimpleNamespace(match_index=f["match_index"], status=f["status"], scores=f["scores"], ind0=f["ind0"], ind1=f["ind1"], live0=int(f["live0"][0]),
                           live1=int(f["live1"][0]), stop_layer=int(f["stop_layer"][0]), layers0=f["layers0"], layers1=f["layers1"])


def _run(ftk, shape, sd, depth, width, min_keypoints=0, c0=None, c1=None, a=None, b=None):
    """(the device's result, the restatement's) of one pass; the inputs must come back untouched."""
    import torch
    m, n, d, h, seed = shape
    a0, b0, kp0, kp1, size = T.inputs(m, n, d, h, seed)
    a, b = (a0 if a is None else a), (b0 if b is None else b)
    lg = _lightglue(ftk, sd, h, depth, width, min_keypoints)
    given = [_cuda(x) for x in (kp0, kp1, a, b)]
    got = lg.match_adaptive(*given, size, size, _count(c0), _count(c1))
    got = _host(got)
    for t, x in zip(given, (kp0, kp1, a, b)):
        assert T.same(t.cpu().numpy(), x), "the call changed an input"
    Wr = _cuda(sd["posenc.Wr.weight"])
    e0, e1 = ftk.rotary_encoding(given[0], size, Wr).cpu().numpy(), ftk.rotary_encoding(given[1], size, Wr).cpu().numpy()
    want = R.run(a, b, h, e0, e1, sd, R.N_LAYERS, depth, width, min_keypoints, c0, c1)
    return got, want


def _mid(shape):
    m, n = shape[:2]
    return (2 * m + 2) // 3, (3 * n + 3) // 4


@pytest.mark.parametrize("counts", ["all_rows", "mid_tile", "zero", "zero_second"])
@pytest.mark.parametrize("steer", ["STOP_AT_0", "STOP_AT_1", "NEVER"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_the_stop_layers_are_the_restatements_bit_for_bit(ftk, shape, steer, counts):
    kwargs, depth, width = getattr(R, steer)
    sd = R.state_dict(shape[2], shape[3], shape[4] + 1000, **kwargs)
    c0, c1 = {"all_rows": (None, None), "mid_tile": _mid(shape), "zero": (0, _mid(shape)[1]), "zero_second": (_mid(shape)[0], 0)}[counts]
    got, want = _run(ftk, shape, sd, depth, width, 0, c0, c1)
    expected = {"STOP_AT_0": 0, "STOP_AT_1": 1, "NEVER": 2}[steer]
    assert want.stop_layer == expected
    n0, n1 = (shape[0] if c0 is None else c0), (shape[1] if c1 is None else c1)
    assert (want.live0, want.live1) == (n0, n1)  # nothing is pruned: confident tokens stop, unsure ones keep every row
    assert R.same_outputs(got, want)


# (at 40 x 70 without the conf term and with one side empty the restatement prunes every row of the other side by layer 1: the condition
# on the inputs below does not hold there, so those two combinations are not cases)
PRUNING_CASES = [(shape, depth_on, counts) for shape in PRUNING_SHAPES for depth_on in (True, False)
                 for counts in ("all_rows", "mid_tile", "zero_first", "zero_second")
                 if not (shape[:2] == (40, 70) and not depth_on and counts.startswith("zero"))]


@pytest.mark.parametrize("shape,depth_on,counts", PRUNING_CASES,
                         ids=["-".join(("x".join(str(v) for v in s[:4]), "with_depth" if d else "width_only", c)) for s, d, c in PRUNING_CASES])
def test_pruning_is_the_restatements_bit_for_bit(ftk, shape, depth_on, counts):
    (a, b, _, _, sd), depth, width = R.prune_case(shape, depth_on)
    c0, c1 = {"all_rows": (None, None), "mid_tile": _mid(shape), "zero_first": (0, _mid(shape)[1]), "zero_second": (_mid(shape)[0], 0)}[counts]
    got, want = _run(ftk, shape, sd, depth, width, 0, c0, c1)
    n0, n1 = (shape[0] if c0 is None else c0), (shape[1] if c1 is None else c1)
    assert want.stop_layer == 2
    for live, given in ((want.live0, n0), (want.live1, n1)):  # the case must prune and keep rows of every side that has any
        assert 1 <= live < given or given == live == 0
    if not depth_on and counts == "all_rows" and shape[:2] in ((65, 130), (130, 65)):
        big, small = (want.live1, want.live0) if shape[0] == 65 else (want.live0, want.live1)
        assert big <= 128 and small <= 32  # a key tile and a row tile are crossed
    assert R.same_outputs(got, want)


def test_pruning_of_one_side_only_with_the_minimum_between_the_counts(ftk):
    shape = R.SHAPES[2]
    (a, b, _, _, sd), depth, width = R.prune_case(shape, True)
    got, want = _run(ftk, shape, sd, depth, width, 100)
    assert want.live0 == 65 and 1 <= want.live1 < 130
    assert R.same_outputs(got, want)


def test_depth_without_width_stops_and_prunes_nothing(ftk):
    shape = R.SHAPES[3]
    kwargs, depth, width = R.DEPTH_ONLY
    got, want = _run(ftk, shape, R.state_dict(shape[2], shape[3], shape[4] + 1000, **kwargs), depth, width)
    assert want.stop_layer == 1 and (want.live0, want.live1) == shape[:2] and (want.layers0 == 2).all()
    assert R.same_outputs(got, want)


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_the_pass_that_never_stops_and_keeps_every_row_equals_match(ftk, shape):
    import torch
    kwargs, depth, width = R.NEVER
    m, n, d, h, seed = shape
    sd = R.state_dict(d, h, seed + 1000, **kwargs)
    a, b, kp0, kp1, size = T.inputs(m, n, d, h, seed)
    lg = _lightglue(ftk, sd, h, depth, width)
    given = [_cuda(x) for x in (kp0, kp1, a, b)]
    c0, c1 = _mid(shape)
    for counts in ((None, None), (_count(c0), _count(c1))):
        scores, index, status = lg.match(*given, size, size, *counts)
        got = lg.match_adaptive(*given, size, size, *counts)
        torch.cuda.synchronize()
        assert int(got.stop_layer[0]) == 2 and np.array_equal(got.ind0.cpu().numpy(), np.arange(m))
        assert T.same(got.scores.cpu().numpy(), scores.cpu().numpy())
        assert np.array_equal(got.match_index.cpu().numpy(), index.cpu().numpy()) and np.array_equal(got.status.cpu().numpy(), status.cpu().numpy())


@pytest.mark.parametrize("dim", [1, 5, 8, 256])
@pytest.mark.parametrize("rows", [1, 32, 33, 129])
def test_confidence_alone(ftk, rows, dim):
    import torch
    from feature_tracker_amd import device as D
    rng = np.random.default_rng(100 * rows + dim)
    n = 7
    x0, x1 = rng.standard_normal((rows, dim)).astype(np.float32), rng.standard_normal((n, dim)).astype(np.float32)
    tw, mw = (4 * rng.standard_normal(dim)).astype(np.float32), (4 * rng.standard_normal(dim)).astype(np.float32)
    tb, mb = np.float32([0.3]), np.float32([-0.7])
    want = [np.concatenate([R.confidence(x0, w, bias[0]), R.confidence(x1, w, bias[0])]) for w, bias in ((tw, tb), (mw, mb))]
    conf, mt = torch.full((rows + n,), 7.0, device="cuda"), torch.full((rows + n,), 7.0, device="cuda")
    D.lightglue_confidence_device(ftk.default_context(), _cuda(x0), _cuda(x1), _cuda(tw), _cuda(tb), _cuda(mw), _cuda(mb), None, None, None, conf, mt)
    torch.cuda.synchronize()
    assert T.same(conf.cpu().numpy(), want[0]) and T.same(mt.cpu().numpy(), want[1])
    live0, live1 = (rows + 1) // 2, 3
    conf.fill_(7.0)
    D.lightglue_confidence_device(ftk.default_context(), _cuda(x0), _cuda(x1), _cuda(tw), _cuda(tb), _cuda(mw), _cuda(mb), _count(live0), _count(live1),
                                  _count(0), conf, mt)
    gated = torch.full((rows + n,), 7.0, device="cuda")
    D.lightglue_confidence_device(ftk.default_context(), _cuda(x0), _cuda(x1), _cuda(tw), _cuda(tb), _cuda(mw), _cuda(mb), None, None, _count(1), gated, gated)
    torch.cuda.synchronize()
    got = conf.cpu().numpy()
    assert T.same(got[:live0], want[0][:live0]) and T.same(got[rows:rows + live1], want[0][rows:rows + live1])
    assert (got[live0:rows] == 7.0).all() and (got[rows + live1:] == 7.0).all() and (gated.cpu().numpy() == 7.0).all()


def test_a_hostile_row_behind_the_live_count_spoils_no_output(ftk):
    shape = R.SHAPES[2]
    (a, b, _, _, sd), depth, width = R.prune_case(shape, True)
    c0, c1 = _mid(shape)
    a, b = np.array(a, copy=True), np.array(b, copy=True)
    a[c0], a[c0 + 1], b[c1, 3], b[c1 + 2] = np.nan, 1e30, np.nan, 1e30
    got, want = _run(ftk, shape, sd, depth, width, 0, c0, c1, a, b)
    assert 1 <= want.live0 < c0 and np.isfinite(want.scores[:want.live0, :want.live1]).all()
    assert R.same_outputs(got, want)


def test_a_captured_graph_replayed_on_descriptors_that_change_the_stop_layer(ftk):
    """Captured on the descriptors, of seven seeded sets, of which the most tokens are confident after layer 0, and replayed on the set of
    which the fewest are; ``depth_confidence`` lies midway between the two ratios (at least 2 / P from either), so the first stops at
    layer 0 and the second, whose tokens are all confident after layer 1, at layer 1."""
    import torch
    shape = R.SHAPES[2]
    m, n, d, h, seed = shape
    steer = R.split_steer(shape)
    sd = R.state_dict(d, h, seed + 1000, token_scale=steer["token_scale"], token_bias=(steer["token_bias"][0], 30.0))
    kp0, kp1, size = T.inputs(m, n, d, h, seed)[2:]
    Wr = _cuda(sd["posenc.Wr.weight"])
    e0, e1 = ftk.rotary_encoding(_cuda(kp0), size, Wr).cpu().numpy(), ftk.rotary_encoding(_cuda(kp1), size, Wr).cpu().numpy()
    sets = [T.inputs(m, n, d, h, seed + k)[:2] for k in range(7)]
    ratios = [1.0 - float((R.run(x, y, h, e0, e1, sd, R.N_LAYERS, -1, -1).conf[0] < R.thresholds(R.N_LAYERS)[0]).mean()) for x, y in sets]
    hi, lo = int(np.argmax(ratios)), int(np.argmin(ratios))
    depth = 0.5 * (ratios[hi] + ratios[lo])
    assert ratios[hi] - ratios[lo] >= 4.0 / (m + n)
    candidates = [sets[hi], sets[lo]]
    wants = [R.run(x, y, h, e0, e1, sd, R.N_LAYERS, depth, -1) for x, y in candidates]
    assert [w.stop_layer for w in wants] == [0, 1]
    first, other = 0, 1
    lg = _lightglue(ftk, sd, h, depth, -1)
    given = [_cuda(x) for x in (kp0, kp1) + tuple(candidates[0])]
    lg.match_adaptive(*given, size, size)  # the buffers are made here, outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        result = lg.match_adaptive(*given, size, size)
    graph.replay()
    assert R.same_outputs(_host(result), wants[0])
    given[2].copy_(torch.from_numpy(np.array(candidates[other][0], copy=True)))
    given[3].copy_(torch.from_numpy(np.array(candidates[other][1], copy=True)))
    graph.replay()
    assert R.same_outputs(_host(result), wants[other]) and wants[other].stop_layer != first


def test_match_adaptive_feeds_the_two_view_filter_on_one_stream(ftk):
    import torch
    from feature_tracker_amd import device as D
    from tests import two_view_ref as TV
    shape = R.SHAPES[2]
    m, n, d, h, seed = shape
    (a, b, _, _, sd), depth, width = R.prune_case(shape, True)
    _, _, kp0, kp1, size = T.inputs(m, n, d, h, seed)
    stream = torch.cuda.Stream()
    ctx = D.context_on_stream(stream)
    with torch.cuda.stream(stream):
        lg = _lightglue(ftk, sd, h, depth, width, ctx=ctx)
        given = [_cuda(x) for x in (kp0, kp1, a, b)]
        got = lg.match_adaptive(*given, size, size, min_score=-20.0)
        cur_uv = given[1][got.match_index.clamp(min=0).long()]
        status = got.status.clone()
        fit = ftk.TwoViewRansac(model="homography", hypotheses=64, threshold=3.0, seed=2, ctx=ctx).filter(given[0], cur_uv, status, (480, 640))
        e0 = ftk.rotary_encoding(given[0], size, _cuda(sd["posenc.Wr.weight"]))
        e1 = ftk.rotary_encoding(given[1], size, _cuda(sd["posenc.Wr.weight"]))
    stream.synchronize()
    want = R.run(a, b, h, e0.cpu().numpy(), e1.cpu().numpy(), sd, R.N_LAYERS, depth, width, min_score=-20.0)
    assert R.same_outputs(_host(got), want)
    want_fit = TV.ransac(kp0, kp1[np.clip(want.match_index, 0, None)], want.status, (480, 640), 3.0, 64, 2, "homography")
    assert np.array_equal(status.cpu().numpy(), want_fit.status) and int(fit.model.item()) == want_fit.model


def test_the_refusals_of_the_library(ftk):
    import torch
    from feature_tracker_amd import _native as N
    ctx = ftk.default_context()
    x = torch.zeros(4096, device="cuda")
    out = torch.full((64,), 7.0, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    conf = lambda m=4, n=4, d=8: N.lib().ftk_lightglue_confidence_device(  # noqa: E731
        ctx.handle, None, p(x), m, p(x), n, d, p(x), p(x), p(x), p(x), None, None, None, p(out), p(out))
    assert conf(m=0) == -1 and conf(n=4097) == -1 and conf(d=0) == -1 and conf(d=1025) == -1
    lay = lambda m=4, n=4, d=8, h=2, live=p(x): N.lib().ftk_transformer_layer_adaptive_device(  # noqa: E731
        ctx.handle, None, p(out), m, p(out), n, d, h, p(x), p(x), p(x), live, p(x), p(x), p(x))
    assert lay(m=0) == -1 and lay(h=3) == -1 and lay(d=6, h=2) == -1 and lay(live=None) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()  # nothing was launched
    with pytest.raises(ValueError, match="token_confidence.0.token.0.weight"):
        _lightglue(ftk, T.state_dict(8, 2, 3, 5), 2, 0.95, -1)
    plain = _lightglue(ftk, T.state_dict(8, 2, 3, 5), 2, -1, -1)
    with pytest.raises(ValueError, match="depth_confidence"):
        plain.match_adaptive(x[:8].view(4, 2), x[:8].view(4, 2), x[:32].view(4, 8), x[:32].view(4, 8), (640, 480), (640, 480))
