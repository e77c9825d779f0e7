"""``attention``, ``TransformerLayer`` and ``LightGlue`` on the device against the scalar restatement (tests/transformer_ref.c, DESIGN.md
5.24): every output element bit for bit, any NaN equal to any NaN."""
import functools

import numpy as np
import pytest

from tests import transformer_ref as R

pytestmark = pytest.mark.gpu

LAYER_IDS = ["x".join(str(v) for v in s[:4]) for s in R.LAYER_SHAPES]
NARROW_IDS = ["x".join(str(v) for v in s[:4]) for s in R.LAYER_NARROW]


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def _count(c):
    import torch
    return None if c is None else torch.tensor([c], dtype=torch.int32, device="cuda")


def _attention(ftk, q, k, v, count=None, **kw):
    """The device's result on the host; the inputs must come back untouched."""
    import torch
    d_q, d_k, d_v = _cuda(q), _cuda(k), _cuda(v)
    out = ftk.attention(d_q, d_k, d_v, _count(count), **kw)
    torch.cuda.synchronize()
    assert R.same(d_q.cpu().numpy(), q) and R.same(d_k.cpu().numpy(), k) and R.same(d_v.cpu().numpy(), v)
    assert tuple(out.shape) == q.shape
    return out.cpu().numpy()


@pytest.mark.parametrize("heads", R.ATTENTION_HEADS, ids=lambda s: f"h{s[0]}dh{s[1]}")
@pytest.mark.parametrize("rows", R.ATTENTION_ROWS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_attention_is_the_restatement_bit_for_bit(ftk, rows, heads):
    (m, n), (h, dh) = rows, heads
    q, k, v = R.qkv(m, n, h, dh, 300 + m + n)
    for count in (None, 0, 1, (n * 7) // 13, n, n + 9, -3):
        assert R.same(_attention(ftk, q, k, v, count), R.attention(q, k, v, count)), ("self form", count)
        pre = R.cross_pre(dh)
        assert R.same(_attention(ftk, q, k, v, count, pre_scale=pre, post_scale=1.0), R.attention(q, k, v, count, pre=pre, post=1.0)), ("cross form", count)
    assert (R.attention(q, k, v, 0) == 0).all() and not np.signbit(R.attention(q, k, v, 0)).any()


@pytest.mark.parametrize("shape", R.ATTENTION_WIDE, ids=lambda s: "x".join(str(v) for v in s))
def test_attention_with_two_and_four_output_tiles_a_wave_and_wide_heads(ftk, shape):
    """The launch shapes of csrc/transformer_plan.cpp beyond one output tile a wave: the same bits."""
    import ctypes as C
    from feature_tracker_amd import _native as N
    m, n, h, dh = shape
    tiles = 1 if -(-m // 32) * h < 256 else (1 if dh <= 32 else 2 if dh <= 64 else 4)  # attention_plan's rule
    assert (tiles > 1) == (m == 1024) and N.lib().ftk_transformer_layer_workspace_bytes(1, 1, h * dh, h, C.byref(C.c_int64())) == 0
    q, k, v = R.qkv(m, n, h, dh, 400 + dh)
    pre = R.cross_pre(dh)
    for count in (None, (n * 7) // 13):
        assert R.same(_attention(ftk, q, k, v, count), R.attention(q, k, v, count)), ("self form", count)
        assert R.same(_attention(ftk, q, k, v, count, pre_scale=pre, post_scale=1.0), R.attention(q, k, v, count, pre=pre, post=1.0)), ("cross form", count)


def test_attention_with_hostile_inputs(ftk):
    m, n, h, dh = 65, 130, 4, 16
    q, k, v = (np.array(x, copy=True) for x in R.qkv(m, n, h, dh, 77))
    v[5, 1, 3] = np.nan
    want = R.attention(q, k, v)
    nan = np.isnan(want)
    assert nan[:, 1, 3].all() and nan.sum() == m  # one output column, nothing else
    assert R.same(_attention(ftk, q, k, v), want)
    q, k, v = (np.array(x, copy=True) for x in R.qkv(m, n, h, dh, 77))
    q[9, 2, 0] = np.nan
    want = R.attention(q, k, v)
    nan = np.isnan(want)
    assert nan[9, 2].all() and nan.sum() == dh  # one row of one head
    assert R.same(_attention(ftk, q, k, v), want)
    q, k, v = (np.array(x, copy=True) for x in R.qkv(m, n, h, dh, 77))
    k[0, 0] = np.inf
    k[3, 1, 2] = -np.inf
    k[70, 2] = 1e30
    k[129, 3] = -1e30
    q[0, 0] = 0.0
    want = R.attention(q, k, v)
    assert np.isnan(want).any() and np.isfinite(want).any()
    assert R.same(_attention(ftk, q, k, v), want)
    assert R.same(_attention(ftk, q, k, v, 70), R.attention(q, k, v, 70))
    pre = R.cross_pre(dh)
    assert R.same(_attention(ftk, q, k, v, 71, pre_scale=pre, post_scale=1.0), R.attention(q, k, v, 71, pre=pre, post=1.0))


def _layer_of(ftk, sd, heads, prefix="transformers.0.", ctx=None):
    import torch
    return ftk.TransformerLayer.from_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, prefix, heads, ctx=ctx)


def _given(shape):
    m, n = shape[:2]
    return (2 * m + 2) // 3, (3 * n + 3) // 4  # some keys invalid (none where there is only one)


@functools.lru_cache(maxsize=None)
def _want(shape, counted):
    a, b, e0, e1, sd = R.layer_case(shape)
    c0, c1 = _given(shape) if counted else (None, None)
    return R.layer(a, b, shape[3], e0, e1, sd, count0=c0, count1=c1)


def _run_layer(layer, a, b, e0, e1, c0=None, c1=None):
    import torch
    d = [_cuda(x) for x in (a, b, e0, e1)]
    out0, out1 = layer(d[0], d[1], d[2], d[3], _count(c0), _count(c1))
    torch.cuda.synchronize()
    for t, x in zip(d, (a, b, e0, e1)):
        assert R.same(t.cpu().numpy(), x), "the call changed an input"
    assert out0.data_ptr() != d[0].data_ptr() and out1.data_ptr() != d[1].data_ptr()
    return out0.cpu().numpy(), out1.cpu().numpy()


@pytest.mark.parametrize("counted", [False, True], ids=["all_rows", "with_counts"])
@pytest.mark.parametrize("shape", R.LAYER_SHAPES + R.LAYER_NARROW, ids=LAYER_IDS + NARROW_IDS)
def test_the_layer_is_the_restatement_bit_for_bit(ftk, shape, counted):
    """LAYER_NARROW: D % 4 != 0, so all eight Linears of the layer run linear_kernel<false> and attention its scalar loads."""
    a, b, e0, e1, sd = R.layer_case(shape)
    c0, c1 = _given(shape) if counted else (None, None)
    got0, got1 = _run_layer(_layer_of(ftk, sd, shape[3]), a, b, e0, e1, c0, c1)
    want0, want1 = _want(shape, counted)
    assert np.isfinite(want0).all() and np.isfinite(want1).all()
    assert R.same(got0, want0) and R.same(got1, want1)


def test_the_layer_with_two_output_tiles_a_wave_and_counts(ftk):
    shape = R.LAYER_WIDE
    a, b, e0, e1, sd = R.layer_case(shape)
    c0, c1 = _given(shape)
    got0, got1 = _run_layer(_layer_of(ftk, sd, shape[3]), a, b, e0, e1, c0, c1)
    want0, want1 = _want(shape, True)
    assert np.isfinite(want0).all() and R.same(got0, want0) and R.same(got1, want1)


def test_a_repeated_call_with_another_size_in_between_gives_the_same_bits(ftk):
    shape, other = R.LAYER_SHAPES[2], R.LAYER_SHAPES[1]
    a, b, e0, e1, sd = R.layer_case(shape)
    layer = _layer_of(ftk, sd, shape[3])
    first = _run_layer(layer, a, b, e0, e1)
    m2, n2 = other[:2]
    _run_layer(layer, a[:m2], b[:n2], np.ascontiguousarray(e0[:, :m2]), np.ascontiguousarray(e1[:, :n2]))  # its own workspace
    second = _run_layer(layer, a, b, e0, e1)
    want = _want(shape, False)
    assert all(R.same(x, y) for x, y in zip(first, second)) and all(R.same(x, y) for x, y in zip(first, want))


def _replayed_graph_equals_the_restatement(ftk, shape, replay_counts):
    import torch
    m, n, d, h, seed = shape
    a, b, e0, e1, sd = R.layer_case(shape)
    a2, b2 = R.inputs(m, n, d, h, seed + 50)[:2]
    layer = _layer_of(ftk, sd, h)
    d_a, d_b, d_e0, d_e1 = (_cuda(x) for x in (a, b, e0, e1))
    c0, c1 = _count(m), _count(n)
    layer(d_a, d_b, d_e0, d_e1, c0, c1)  # the workspace is made here, outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out0, out1 = layer(d_a, d_b, d_e0, d_e1, c0, c1)
    d_a.copy_(torch.from_numpy(a2.copy()))
    d_b.copy_(torch.from_numpy(b2.copy()))
    c0.fill_(replay_counts[0])
    c1.fill_(replay_counts[1])
    graph.replay()
    torch.cuda.synchronize()
    want0, want1 = R.layer(a2, b2, h, e0, e1, sd, count0=replay_counts[0], count1=replay_counts[1])
    assert R.same(out0.cpu().numpy(), want0) and R.same(out1.cpu().numpy(), want1)


def test_a_captured_graph_replayed_on_changed_descriptors_and_counts_equals_the_restatement(ftk):
    _replayed_graph_equals_the_restatement(ftk, R.LAYER_SHAPES[2], (40, 101))


def test_a_captured_graph_of_the_non_vector_path_replayed_equals_the_restatement(ftk):
    shape = R.LAYER_NARROW[3]
    assert shape[:4] == (40, 70, 18, 3)
    _replayed_graph_equals_the_restatement(ftk, shape, (25, 43))


def _offset_by_one_float(array_or_shape):
    """A contiguous CUDA view one float into a larger tensor, so only 4-byte aligned; the tensor it lies in."""
    import torch
    given = isinstance(array_or_shape, np.ndarray)
    shape = array_or_shape.shape if given else tuple(array_or_shape)
    big = torch.full((int(np.prod(shape)) + 1,), 7.0, dtype=torch.float32, device="cuda")
    view = big[1:].view(shape)
    if given:
        view.copy_(torch.from_numpy(np.array(array_or_shape, copy=True)))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view, big


@pytest.mark.parametrize("offset", ["desc0", "desc1", "weights", "out0", "out1", "all_five"])
def test_the_layer_on_buffers_that_are_only_4_byte_aligned(ftk, offset):
    """D % 4 == 0, so the alignment alone selects linear_kernel<false> and attention's scalar loads: each of the five buffers the entry
    looks at, and then all of them, one float into a larger tensor.  The torch entry takes such views; the bits are the restatement's,
    which are the aligned run's, with and without counts, and the float in front of each view keeps its value."""
    import torch
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    shape = R.LAYER_SHAPES[2]
    m, n, d, h, _ = shape
    a, b, e0, e1, sd = R.layer_case(shape)
    packed = next(iter(_layer_of(ftk, sd, h)._packed.values())).numpy()
    moved = ("desc0", "desc1", "weights", "out0", "out1") if offset == "all_five" else (offset,)
    for counted in (False, True):
        given = dict(desc0=a, desc1=b, weights=packed, out0=(m, d), out1=(n, d))
        t, fronts = {}, []
        for name, value in given.items():
            if name in moved:
                t[name], big = _offset_by_one_float(value)
                fronts.append(big)
            else:
                t[name] = _cuda(value) if isinstance(value, np.ndarray) else torch.empty(value, dtype=torch.float32, device="cuda")
                assert t[name].data_ptr() % 16 == 0
        enc0, enc1 = _cuda(e0), _cuda(e1)
        c0, c1 = _given(shape) if counted else (None, None)
        workspace = torch.empty(-(-N.transformer_layer_workspace_bytes(m, n, d, h) // 8), dtype=torch.int64, device="cuda")
        D.transformer_layer_device(ftk.default_context(), t["desc0"], t["desc1"], h, enc0, enc1, t["weights"], _count(c0), _count(c1), workspace,
                                   t["out0"], t["out1"])
        torch.cuda.synchronize()
        want0, want1 = _want(shape, counted)
        assert R.same(t["out0"].cpu().numpy(), want0) and R.same(t["out1"].cpu().numpy(), want1), (offset, counted)
        assert R.same(t["desc0"].cpu().numpy(), a) and R.same(t["desc1"].cpu().numpy(), b) and R.same(t["weights"].cpu().numpy(), packed)
        assert all(float(big[0]) == 7.0 for big in fronts)


@functools.lru_cache(maxsize=None)
def _want_scaled(counted):
    shape = R.LAYER_SHAPES[2]
    a, b, e0, e1, sd = R.scaled_gelu_case(shape)
    c0, c1 = _given(shape) if counted else (None, None)
    return R.layer(a, b, shape[3], e0, e1, sd, count0=c0, count1=c1)


@pytest.mark.parametrize("counted", [False, True], ids=["all_rows", "with_counts"])
def test_the_layer_with_every_branch_of_erf_c_taken(ftk, counted):
    """Both blocks' LayerNorm weight times 6: about 19 % / 47 % / 34 % of the self block's pre-GELU values fall in erf_c's branches
    a < 1, 1 <= a < 4 and a >= 4 (at least 1 % each is asserted here and, with the float64 pin, in tests/test_transformer_cpu.py); with
    the weights as they are the last branch is never taken."""
    shape = R.LAYER_SHAPES[2]
    a, b, e0, e1, sd = R.scaled_gelu_case(shape)
    c0, c1 = _given(shape) if counted else (None, None)
    assert min(R.erf_branch_shares(R.self_block_pre_gelu(a, shape[3], e0, sd, c0))) >= 0.01
    want0, want1 = _want_scaled(counted)
    assert np.isfinite(want0).all() and np.isfinite(want1).all()
    got0, got1 = _run_layer(_layer_of(ftk, sd, shape[3]), a, b, e0, e1, c0, c1)
    assert R.same(got0, want0) and R.same(got1, want1)


def test_the_layer_with_hostile_rows_behind_the_counts(ftk):
    """NaN, inf, zeros, subnormals, 1e30 and 3e38 rows behind the counts (transformer_ref.hostile_layer_case): attention masks them as
    keys, so they spoil only themselves.  On the restatement: NaN rows and finite rows in both sets, one NaN row that entered finite
    (3e38: its Linears overflow), and the 1e30 row, whose LayerNorm variance overflows to inf (rstd = 0), finite.  Then the device, bit for bit."""
    shape = R.LAYER_SHAPES[2]
    a, b, e0, e1, sd = R.hostile_layer_case(shape)
    c0, c1 = R.HOSTILE_COUNTS
    want0, want1 = R.layer(a, b, shape[3], e0, e1, sd, count0=c0, count1=c1)
    nan0, nan1 = np.isnan(want0).all(1), np.isnan(want1).all(1)
    assert nan0.sum() == 1 and nan1.sum() == 2 and np.isfinite(want0[~nan0]).all() and np.isfinite(want1[~nan1]).all()
    assert nan1[8] and np.isfinite(b[8]).all() and np.isfinite(want1[7]).all() and (b[7] == np.float32(1e30)).all()
    got0, got1 = _run_layer(_layer_of(ftk, sd, shape[3]), a, b, e0, e1, c0, c1)
    assert R.same(got0, want0) and R.same(got1, want1)


def test_lightglue_is_the_restatements_composed_and_feeds_the_two_view_filter_without_a_host_read(ftk):
    """LightGlue with two layers and an input projection: ``scores`` equal linear, layer, layer and the assignment head's restatement
    composed; ``match`` and TwoViewRansac run on one stream with nothing read on the host before the final comparison."""
    import torch
    from feature_tracker_amd import device as D
    from tests import match_assignment_ref as MA
    from tests import nn_match_ref
    from tests import two_view_ref as T
    m, n, d, h, seed = R.LAYER_SHAPES[2]
    d_in = 24
    sd = R.state_dict(d, h, 2, 901, d_in)
    rng = np.random.default_rng(902)
    _, _, kp0, kp1, size = R.inputs(m, n, d, h, seed)
    raw0, raw1 = rng.standard_normal((m, d_in)).astype(np.float32), rng.standard_normal((n, d_in)).astype(np.float32)
    c0, c1, min_score = 60, 111, -20.0
    stream = torch.cuda.Stream()
    ctx = D.context_on_stream(stream)
    with torch.cuda.stream(stream):
        lg = ftk.LightGlue.from_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, num_heads=h, ctx=ctx)
        assert len(lg.layers) == 2 and lg.dim == d
        args = [_cuda(x) for x in (kp0, kp1, raw0, raw1)]
        count0, count1 = _count(c0), _count(c1)
        scores_only = lg.scores(*args, size, size, count0, count1)
        scores, index, status = lg.match(*args, size, size, count0, count1, min_score=min_score)
        cur_uv = args[1][index.clamp(min=0).long()]
        before = status.clone()
        fit = ftk.TwoViewRansac(model="homography", hypotheses=64, threshold=3.0, seed=2, ctx=ctx).filter(args[0], cur_uv, status, (480, 640))
        enc0, enc1 = ftk.rotary_encoding(args[0], size, _cuda(sd["posenc.Wr.weight"])), ftk.rotary_encoding(args[1], size, _cuda(sd["posenc.Wr.weight"]))
    stream.synchronize()
    # ---- the final comparison; the encoding is an input of the contract, so the restatement takes the device's ----
    e0, e1 = enc0.cpu().numpy(), enc1.cpu().numpy()
    assert e0.shape == (2, m, d // h) and np.abs(e0 - R.encoding(kp0, size, sd["posenc.Wr.weight"])).max() < 1e-5
    x0, x1 = R.linear(raw0, sd["input_proj.weight"], sd["input_proj.bias"]), R.linear(raw1, sd["input_proj.weight"], sd["input_proj.bias"])
    for i in range(2):
        x0, x1 = R.layer(x0, x1, h, e0, e1, sd, f"transformers.{i}.", c0, c1)
    w, bias = MA.pack(*(sd[f"log_assignment.1.{k}"] for k in ("final_proj.weight", "final_proj.bias", "matchability.weight", "matchability.bias")))
    want = MA.assign(x0, x1, weights=w, bias=bias, count0=c0, count1=c1)
    assert R.same(scores.cpu().numpy(), want) and R.same(scores_only.cpu().numpy(), want)
    want_index, want_status = nn_match_ref.match_scores(want[:m, :n], min_score)
    assert np.array_equal(index.cpu().numpy(), want_index) and np.array_equal(before.cpu().numpy(), want_status)
    assert (want_index[c0:] == -1).all() and (want_index < c1).all()
    want_fit = T.ransac(kp0, kp1[np.clip(want_index, 0, None)], want_status, (480, 640), 3.0, 64, 2, "homography")
    assert np.array_equal(status.cpu().numpy(), want_fit.status) and int(fit.model.item()) == want_fit.model


def test_the_refusals_of_the_library(ftk):
    import torch
    from feature_tracker_amd import _native as N
    ctx = ftk.default_context()
    x = torch.zeros(8, 8, device="cuda")
    out = torch.full((8, 8), 7.0, device="cuda")
    ws = torch.zeros(4096, dtype=torch.int64, device="cuda")
    att = lambda m=8, n=8, h=2, dh=4, pre=1.0, post=0.5: N.lib().ftk_attention_device(  # noqa: E731
        ctx.handle, None, x.data_ptr(), m, x.data_ptr(), x.data_ptr(), n, h, dh, None, pre, post, out.data_ptr())
    assert att(m=0) == -1 and att(n=4097) == -1 and att(h=0) == -1 and att(dh=3) == -1 and att(dh=130) == -1 and att(h=1024, dh=2) == -1
    assert att(pre=0.0) == -1 and att(post=float("nan")) == -1 and att(post=float("inf")) == -1
    lay = lambda m=4, n=4, d=8, h=2: N.lib().ftk_transformer_layer_device(  # noqa: E731
        ctx.handle, None, x.data_ptr(), m, x.data_ptr(), n, d, h, x.data_ptr(), x.data_ptr(), x.data_ptr(), None, None, ws.data_ptr(), out.data_ptr(),
        out.data_ptr())
    assert lay(m=0) == -1 and lay(n=4097) == -1 and lay(d=1028, h=257) == -1 and lay(h=3) == -1 and lay(d=6, h=2) == -1 and lay(d=0) == -1
    lin = lambda rows=8, k=8, o=8: N.lib().ftk_linear_device(ctx.handle, None, x.data_ptr(), rows, k, x.data_ptr(), x.data_ptr(), o, out.data_ptr())  # noqa: E731
    assert lin(rows=0) == -1 and lin(k=0) == -1 and lin(o=1025) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()  # nothing was launched
    assert att() == 0
