"""The loud failures of the transformer layer before any device is touched: the walk of tests/args_walk.py over
``device.attention_device``, ``device.linear_device`` and ``device.transformer_layer_device``; the refusals of ``attention``,
``TransformerLayer`` and ``LightGlue``; the agreement of header, library and binding; and the launch plan through
host/build/transformer_plan_cli."""
import types

import pytest

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

PLAN_CLI = A.plan_cli("transformer_plan_cli")


def _layer(w, m=6, n=7, d=16, h=4, counts=True):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    dh = d // h if isinstance(h, int) and h > 0 else 1
    clip = lambda v, hi: min(max(v, 1), hi)  # noqa: E731
    words = 8 * (clip(m, 4096) + clip(n, 4096)) * clip(d, 1024) // 2 + 8  # (enough for every refused shape too)
    return D.transformer_layer_device(w.ctx, w.t("desc0", "float32", m, d), w.t("desc1", "float32", n, d), h, w.t("enc0", "float32", 2, m, dh),
                                      w.t("enc1", "float32", 2, n, dh), w.t("weights", "float32", N.transformer_layer_weight_offsets(d)[2]),
                                      w.t("count0", "int32", 1) if counts else None, w.t("count1", "int32", 1) if counts else None,
                                      w.t("workspace", "int64", words), w.t("out0", "float32", m, d), w.t("out1", "float32", n, d))


def _attention(w, m=6, n=7, h=2, dh=8, count=True, pre=1.0, post=None):
    from feature_tracker_amd import device as D
    return D.attention_device(w.ctx, w.t("q", "float32", m, h, dh), w.t("k", "float32", n, h, dh), w.t("v", "float32", n, h, dh),
                              w.t("count", "int32", 1) if count else None, pre, post, w.t("out", "float32", m, h, dh))


def _linear(w, rows=6, k=5, o=9):
    from feature_tracker_amd import device as D
    return D.linear_device(w.ctx, w.t("x", "float32", rows, k), w.t("weight", "float32", o, k), w.t("bias", "float32", o), w.t("out", "float32", rows, o))


CALLS = {"ftk_transformer_layer_device": _layer, "ftk_attention_device": _attention, "ftk_linear_device": _linear}


@pytest.mark.parametrize("native", sorted(CALLS))
def test_entry_takes_no_pointer_of_an_unchecked_argument(monkeypatch, native):
    A.walk_call(monkeypatch, CALLS[native], [native])


@pytest.mark.parametrize("kind", ["dtype", "device"])
@pytest.mark.parametrize("native", sorted(CALLS))
def test_each_refused_tensor_stops_the_entry_before_the_library(monkeypatch, native, kind):
    A.refusal_sweep(monkeypatch, CALLS[native], kind)


def test_other_refusals(monkeypatch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    w = A.Walk(monkeypatch)
    for match, call, kw in (("FTK_TRANSFORMER_MAX_ROWS", _layer, dict(m=4097)), ("FTK_TRANSFORMER_MAX_ROWS", _layer, dict(n=0)),
                            ("FTK_TRANSFORMER_MAX_DIM", _layer, dict(d=1028, h=257)), ("must divide D", _layer, dict(d=16, h=3)),
                            ("FTK_TRANSFORMER_MAX_HEAD_DIM", _layer, dict(d=6, h=2)), ("FTK_TRANSFORMER_MAX_HEAD_DIM", _layer, dict(d=260, h=2)),
                            ("num_heads must be a positive integer", _layer, dict(h=0)), ("num_heads must be", _layer, dict(h=4.0)),
                            ("FTK_TRANSFORMER_MAX_ROWS", _attention, dict(m=4097)), ("FTK_TRANSFORMER_MAX_HEAD_DIM", _attention, dict(dh=3)),
                            ("FTK_TRANSFORMER_MAX_HEAD_DIM", _attention, dict(dh=130)), ("FTK_TRANSFORMER_MAX_DIM", _attention, dict(h=16, dh=128)),
                            ("pre_scale must be a finite number > 0", _attention, dict(pre=0.0)), ("post_scale must be", _attention, dict(post=float("nan"))),
                            ("post_scale must be", _attention, dict(post="big")), ("FTK_TRANSFORMER_MAX_ROWS", _linear, dict(rows=4097)),
                            ("FTK_TRANSFORMER_MAX_DIM", _linear, dict(k=1025)), ("FTK_TRANSFORMER_MAX_DIM", _linear, dict(o=1025))):
        with pytest.raises(ValueError, match=match):
            call(w, **kw)
    assert w.lib.calls == [] and w.unchecked_reads == []
    for call, kw in ((_layer, dict()), (_layer, dict(counts=False)), (_layer, dict(m=1, n=1, d=4, h=2)), (_layer, dict(m=4096, n=4096, d=4, h=2)),
                     (_layer, dict(d=1024, h=8)), (_attention, dict(count=False)), (_attention, dict(dh=128, post=0.25)), (_linear, dict(k=1024, o=1024))):
        call(w, **kw)
    assert len(w.lib.calls) == 8
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    d, h = 16, 4
    sd = {}
    for block, names in (("self_attn", (("Wqkv", 3 * d, d), ("out_proj", d, d))), ("cross_attn", (("to_qk", d, d), ("to_v", d, d), ("to_out", d, d)))):
        for name, outs, ins in names + (("ffn.0", 2 * d, 2 * d), ("ffn.3", d, 2 * d)):
            sd[f"transformers.0.{block}.{name}.weight"], sd[f"transformers.0.{block}.{name}.bias"] = torch.zeros(outs, ins), torch.zeros(outs)
        sd[f"transformers.0.{block}.ffn.1.weight"], sd[f"transformers.0.{block}.ffn.1.bias"] = torch.ones(2 * d), torch.zeros(2 * d)
    # the repacking: upstream's Wqkv row (a dh + e) 3 + t becomes row t D + a dh + e
    sd["transformers.0.self_attn.Wqkv.weight"] = torch.arange(3 * d, dtype=torch.float32).unsqueeze(1).repeat(1, d)
    layer = F.TransformerLayer.from_state_dict(sd, num_heads=h)
    packed = next(iter(layer._packed.values()))
    assert layer.dim == d and layer.head_dim == 4 and packed.numel() == N.transformer_layer_weight_offsets(d)[2] and packed.is_contiguous()
    assert packed[:3 * d * d].view(3, d, d)[:, :, 0].tolist() == [[3.0 * c + t for c in range(d)] for t in range(3)]
    assert F.TransformerLayer.from_state_dict({k.replace("transformers.0.", "layer."): v for k, v in sd.items()}, prefix="layer.", num_heads=2).head_dim == 8
    for match, change, heads in (("lacks", {"transformers.0.cross_attn.to_v.bias": None}, h),
                                 ("must be a float32 tensor", {"transformers.0.self_attn.out_proj.weight": torch.zeros(d, d).double()}, h),
                                 ("Wqkv.weight must be \\[3 D, D\\]", {"transformers.0.self_attn.Wqkv.weight": torch.zeros(2 * d, d)}, h),
                                 ("ffn.0.weight must be \\[32, 32\\]", {"transformers.0.cross_attn.ffn.0.weight": torch.zeros(2 * d, d)}, h),
                                 ("ffn.1.bias must be \\[32\\]", {"transformers.0.self_attn.ffn.1.bias": torch.zeros(d)}, h), ("must divide D", {}, 3),
                                 ("FTK_TRANSFORMER_MAX_HEAD_DIM", {}, 16)):
        bad = {k: v for k, v in {**sd, **change}.items() if v is not None}
        with pytest.raises(ValueError, match=match):
            F.TransformerLayer.from_state_dict(bad, num_heads=heads)
    with pytest.raises(ValueError, match="context_on_stream"):
        F.TransformerLayer.from_state_dict(sd, num_heads=h, ctx=types.SimpleNamespace(handle=None))
    a, b, e0, e1 = torch.zeros(6, d), torch.zeros(7, d), torch.zeros(2, 6, 4), torch.zeros(2, 7, 4)
    one = torch.zeros(1, dtype=torch.int32)
    for match, args, kw in (("^desc0 must be .*wrong dtype", (a.double(), b, e0, e1), {}), ("^desc1 must be .*dimension 1 is 15", (a, torch.zeros(7, 15), e0, e1), {}),
                            ("^desc0 must be .*strided view", (torch.zeros(6, 32)[:, ::2], b, e0, e1), {}), ("^enc0 must be .*dimension 1 is 5", (a, b, torch.zeros(2, 5, 4), e1), {}),
                            ("^enc1 must be .*dimension 2 is 8", (a, b, e0, torch.zeros(2, 7, 8)), {}), ("^count0 must be .*wrong dtype", (a, b, e0, e1), dict(count0=one.long())),
                            ("FTK_TRANSFORMER_MAX_ROWS", (torch.zeros(4097, d), b, torch.zeros(2, 4097, 4), e1), {}), ("no CPU fallback", (a, b, e0, e1), {}),
                            ("no CPU fallback", (a, b, e0, e1), dict(count0=one, count1=one))):
        with pytest.raises(ValueError, match=match):
            layer(*args, **kw)
    q, k = torch.zeros(6, 2, 8), torch.zeros(7, 2, 8)
    for match, args, kw in (("^q must be .*2 dimensions instead of 3", (torch.zeros(6, 16), k, k), {}), ("^k must be .*dimension 2 is 4", (q, torch.zeros(7, 2, 4), k), {}),
                            ("^v must be .*dimension 0 is 6", (q, k, torch.zeros(6, 2, 8)), {}), ("^count must be", (q, k, k), dict(count=one.long())),
                            ("no CPU fallback", (q, k, k), {})):
        with pytest.raises(ValueError, match=match):
            F.attention(*args, **kw)
    head = {"log_assignment.0.final_proj.weight": torch.zeros(d, d), "log_assignment.0.final_proj.bias": torch.zeros(d),
            "log_assignment.0.matchability.weight": torch.zeros(1, d), "log_assignment.0.matchability.bias": torch.zeros(1)}
    full = {**sd, **head, "posenc.Wr.weight": torch.zeros(2, 2)}
    lg = F.LightGlue.from_state_dict(full, num_heads=h)
    assert len(lg.layers) == 1 and lg.input_proj is None and lg.head.dim == d
    with_proj = F.LightGlue.from_state_dict({**full, "input_proj.weight": torch.zeros(d, 24), "input_proj.bias": torch.zeros(d)}, num_heads=h)
    assert tuple(with_proj.input_proj[0].shape) == (d, 24)
    for match, change, kw in (("posenc.Wr.weight", {"posenc.Wr.weight": None}, {}), ("posenc.Wr.weight must be a float32 tensor of shape \\[2, 2\\]", {"posenc.Wr.weight": torch.zeros(4, 2)}, {}),
                              ("n_layers must be a positive integer", {}, dict(n_layers=0)), ("lacks", {}, dict(n_layers=2)),
                              ("input_proj.weight must be \\[16", {"input_proj.weight": torch.zeros(8, 24), "input_proj.bias": torch.zeros(d)}, {})):
        bad = {k: v for k, v in {**full, **change}.items() if v is not None}
        with pytest.raises(ValueError, match=match):
            F.LightGlue.from_state_dict(bad, num_heads=h, **kw)
    kp0, kp1 = torch.zeros(6, 2), torch.zeros(7, 2)
    for match, args in (("^desc0 must be .*dimension 1 is 24", (kp0, kp1, torch.zeros(6, 24), b)), ("^kpts0 must be .*dimension 0 is 5", (torch.zeros(5, 2), kp1, a, b)),
                        ("no CPU fallback", (kp0, kp1, a, b))):
        with pytest.raises(ValueError, match=match):
            lg.scores(*args, (640, 480), (640, 480))
    with pytest.raises(ValueError, match="no CPU fallback"):
        lg.match(kp0, kp1, a, b, (640, 480), (640, 480), min_score=-3.0)
    for match, call in (("min_score must be a number", lambda: lg.match(kp0, kp1, a, b, (640, 480), (640, 480), min_score=float("nan"))),
                        ("size0 must be \\(width, height\\)", lambda: lg.scores(kp0, kp1, a, b, (640, 0), (640, 480))),
                        ("size1 must be", lambda: lg.scores(kp0, kp1, a, b, (640, 480), 640)), ("size1 must be", lambda: lg.match(kp0, kp1, a, b, (640, 480), (640, float("inf"))))):
        with pytest.raises(ValueError, match=match):
            call()
    assert all(layer._workspace is with_proj._workspace for layer in with_proj.layers)  # one workspace for the whole composition
    for match, args in (("FTK_TRANSFORMER_MAX_ROWS", (4097, 1, 4, 2)), ("FTK_TRANSFORMER_MAX_DIM", (1, 1, 1028, 257)), ("must divide", (1, 1, 7, 2)),
                        ("FTK_TRANSFORMER_MAX_HEAD_DIM", (1, 1, 6, 2)), ("FTK_TRANSFORMER_MAX_HEAD_DIM", (1, 1, 260, 2))):
        with pytest.raises(ValueError, match=match):
            N.transformer_layer_workspace_bytes(*args)
    enc = F.rotary_encoding(torch.tensor([[320.0, 240.0], [640.0, 480.0]]), (640, 480), torch.tensor([[1.0, 0.0], [0.0, 2.0]]))
    assert tuple(enc.shape) == (2, 2, 4) and enc[0, 0].tolist() == [1.0] * 4 and enc[1, 0].tolist() == [0.0] * 4
    assert torch.equal(enc[0, 1], torch.cos(torch.tensor([1.0, 1.0, 1.5, 1.5]))) and torch.equal(enc[1, 1], torch.sin(torch.tensor([1.0, 1.0, 1.5, 1.5])))
    assert recorder.calls == []


def test_header_library_and_binding_agree():
    import ctypes as C
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    A.header_library_and_binding_agree(("FTK_TRANSFORMER_MAX_ROWS", "FTK_TRANSFORMER_MAX_DIM", "FTK_TRANSFORMER_MAX_HEAD_DIM"),
                                       {"ftk_transformer_layer_workspace_bytes", "ftk_attention_device", "ftk_linear_device", "ftk_transformer_layer_device"})
    assert {"TransformerLayer", "LightGlue", "attention", "rotary_encoding"} <= set(F.__all__)
    assert callable(D.attention_device) and callable(D.linear_device) and callable(D.transformer_layer_device)
    lib, out = N.lib(), C.c_int64()
    for m, n in ((1, 1), (31, 33), (64, 65), (300, 2048), (4096, 4096)):
        for d, h in ((4, 2), (6, 1), (64, 4), (256, 4), (1024, 8)):
            assert lib.ftk_transformer_layer_workspace_bytes(m, n, d, h, C.byref(out)) == 0
            assert out.value == N.transformer_layer_workspace_bytes(m, n, d, h) and out.value % 16 == 0
    bytes_of = lib.ftk_transformer_layer_workspace_bytes
    assert bytes_of(0, 1, 4, 2, C.byref(out)) == -1 and bytes_of(1, 4097, 4, 2, C.byref(out)) == -1 and bytes_of(1, 1, 1028, 257, C.byref(out)) == -1
    assert bytes_of(1, 1, 6, 2, C.byref(out)) == -1 and bytes_of(1, 1, 260, 2, C.byref(out)) == -1 and bytes_of(1, 1, 7, 2, C.byref(out)) == -1
    assert bytes_of(1, 1, 4, 0, C.byref(out)) == -1 and bytes_of(1, 1, 4, 2, None) == -1
    assert lib.ftk_transformer_layer_device(None, None, None, 1, None, 1, 4, 2, None, None, None, None, None, None, None, None) == -1  # null context
    assert lib.ftk_attention_device(None, None, None, 1, None, None, 1, 2, 2, None, 1.0, 1.0, None) == -1
    assert lib.ftk_linear_device(None, None, None, 1, 1, None, None, 1, None) == -1


def test_nothing_in_the_package_imports_the_restatement():
    A.nothing_in_the_package_imports("transformer_ref")


def _plan(m, n, d, h, aligned):
    """The plan restated (csrc/transformer_plan.cpp)."""
    if not (1 <= m <= 4096 and 1 <= n <= 4096):
        return {"refused": "rows"}
    if not 1 <= d <= 1024:
        return {"refused": "dim"}
    if h < 1 or d % h != 0:
        return {"refused": "heads"}
    dh = d // h
    if dh % 2 != 0 or not 2 <= dh <= 128:
        return {"refused": "head_dim"}
    up16 = lambda v: (v + 15) & ~15  # noqa: E731
    r = m + n
    vec = int(d % 4 == 0 and bool(aligned))
    grid_x = -(-max(m, n) // 32)
    out_tiles = (1 if dh <= 32 else 2 if dh <= 64 else 4) if grid_x * h * 2 >= 256 else 1
    plan = {"refused": "none", "head_dim": dh, "vec_linear": vec, "vec_attn": int(vec and dh % 4 == 0), "linear_threads": 256, "linear_grid_x": -(-r // 128),
            "grid_y_d": -(-d // 128), "grid_y_2d": -(-2 * d // 128), "grid_y_3d": -(-3 * d // 128), "attn_threads": 64, "attn_out_tiles": out_tiles,
            "attn_grid_x": grid_x, "attn_grid_y": h * -(-dh // (32 * out_tiles)), "attn_grid_z": 2, "norm_threads": 64, "norm_blocks": r,
            "launches": 12, "off_qkv": 0, "off_ctx": up16(12 * r * d)}
    plan["off_msg"] = plan["off_ctx"] + up16(4 * r * d)
    plan["off_hidden"] = plan["off_msg"] + up16(4 * r * d)
    plan["off_x1"] = plan["off_hidden"] + up16(8 * r * d)
    plan["bytes"] = plan["off_x1"] + up16(4 * r * d)
    at = 0
    for block, in_outs in (("self", 3 * d), ("cross", 2 * d)):
        for k, size in enumerate((in_outs * d, in_outs, d * d, d, 4 * d * d, 2 * d, 2 * d, 2 * d, 2 * d * d, d)):
            plan[f"w_{block}{k}"] = at
            at += size
    plan["weight_floats"] = at
    return plan


def test_the_shapes_of_the_non_vector_gpu_tests_plan_the_non_vector_kernels():
    """What tests/test_transformer_gpu.py relies on: every LAYER_NARROW shape plans the non-vector Linear and attention whatever the
    alignment; LAYER_SHAPES[2] plans them only for buffers that are not 16-byte aligned; D = 130 has the column tiles it is there for;
    and the Linear's row tile is the header's kLinearTileRows, which LINEAR_ROWS brackets."""
    from tests import transformer_ref as R
    tile = R.linear_tile_rows()
    assert R.LINEAR_ROWS == (1, 31, 32, 33, tile - 1, tile, tile + 1)
    cases = [s[:4] + (1,) for s in R.LAYER_NARROW] + [R.LAYER_SHAPES[2][:4] + (0,), R.LAYER_SHAPES[2][:4] + (1,), (tile - 1, 1, 8, 2, 1), (tile, 1, 8, 2, 1)]
    plans = A.run_plan_tool(PLAN_CLI, cases)
    assert all(p["refused"] == "none" for p in plans)
    k = len(R.LAYER_NARROW)
    assert all(s[2] % 4 != 0 for s in R.LAYER_NARROW) and all((p["vec_linear"], p["vec_attn"]) == ("0", "0") for p in plans[:k])
    assert R.LAYER_NARROW[4][2] == 130 and [plans[4][f"grid_y_{c}"] for c in ("d", "2d", "3d")] == ["2", "3", "4"]
    assert (plans[k]["vec_linear"], plans[k]["vec_attn"]) == ("0", "0") and (plans[k + 1]["vec_linear"], plans[k + 1]["vec_attn"]) == ("1", "1")
    assert plans[k + 2]["linear_grid_x"] == "1" and plans[k + 3]["linear_grid_x"] == "2" and int(plans[k]["linear_threads"]) == 2 * tile


def test_plan_cli_equals_the_restated_plan():
    from feature_tracker_amd import _native as N
    cases = [(m, n, d, h, aligned) for m, n in ((1, 1), (31, 33), (65, 130), (300, 300), (1024, 1000), (2048, 2048), (4096, 4096), (4097, 1), (1, 4097), (0, 5), (-1, -1))
             for d, h in ((4, 2), (6, 1), (6, 3), (8, 2), (64, 4), (256, 4), (256, 2), (1024, 8), (1024, 16), (6, 2), (260, 2), (7, 2), (256, 3), (0, 1), (1025, 5), (4, 0), (8, 8))
             for aligned in (0, 1)]
    plans = A.run_plan_tool(PLAN_CLI, cases)
    seen = set()
    for case, got in zip(cases, plans):
        want = _plan(*case)
        assert got == {k: str(v) for k, v in want.items()}, (case, got, want)
        seen.add(want["refused"])
        if want["refused"] == "none":
            assert want["bytes"] == N.transformer_layer_workspace_bytes(*case[:4])
            offsets = N.transformer_layer_weight_offsets(case[2])
            assert [want[f"w_self{k}"] for k in range(10)] == list(offsets[0]) and [want[f"w_cross{k}"] for k in range(10)] == list(offsets[1])
            assert want["weight_floats"] == offsets[2] and want["attn_grid_y"] <= 65535
    assert seen == {"none", "rows", "dim", "heads", "head_dim"}
