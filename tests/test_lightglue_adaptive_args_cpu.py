"""The adaptive pass without a device: the plan equal to its Python restatement through
host/build/lightglue_adaptive_plan_cli at the limit edges; header, library and binding in agreement; tensors refused before the library."""
import ctypes as C
import os
import re

import pytest

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

PLAN_CLI = A.plan_cli("lightglue_adaptive_plan_cli")
ENTRIES = ("ftk_lightglue_adaptive_workspace_bytes", "ftk_transformer_layer_adaptive_device", "ftk_lightglue_confidence_device",
           "ftk_lightglue_adapt_step_device", "ftk_lightglue_finish_device")


def _restated(m, n, d, h):
    """csrc/lightglue_adaptive_plan.cpp in Python: None where it refuses."""
    from feature_tracker_amd import _native as N
    try:
        layer = N.transformer_layer_workspace_bytes(m, n, d, h)
    except ValueError:
        return None
    up16 = lambda v: (v + 15) & ~15  # noqa: E731
    tiles = lambda v, per: -(-v // per)  # noqa: E731
    p = dict(conf_threads=64, conf_blocks=tiles(m + n, 64), decide_threads=256, decide_blocks=1, gather_threads=64, gather_blocks=m + n, copy_threads=256,
             select_blocks=min(tiles((d + 1) * d + d + 1 + m, 256), 1024), remap_blocks=tiles(m + n, 256), step_launches=3, finish_launches=2, off_layer=0)
    p["off_assign"] = up16(layer)
    p["off_head_w"] = p["off_assign"] + up16(N.match_assignment_workspace_bytes(m, n, d, True))
    p["off_head_b"] = p["off_head_w"] + up16(4 * (d + 1) * d)
    p["off_src0"] = p["off_head_b"] + up16(4 * (d + 1))
    p["off_src1"] = p["off_src0"] + up16(4 * m)
    p["off_match"] = p["off_src1"] + up16(4 * n)
    p["off_status"] = p["off_match"] + up16(4 * m)
    p["bytes"] = p["off_status"] + up16(m)
    return p


def test_plan_cli_equals_the_restated_plan_at_every_limit_edge():
    from feature_tracker_amd import _native as N
    cases = [(m, n, d, h) for m, n in ((1, 1), (33, 31), (65, 130), (255, 257), (300, 300), (4096, 4096), (4097, 1), (1, 4097), (0, 5), (-1, -1))
             for d, h in ((4, 2), (8, 2), (18, 3), (64, 4), (256, 4), (1024, 8), (1024, 16), (6, 2), (256, 3), (0, 1), (1025, 5), (4, 0))]
    plans = A.run_plan_tool(PLAN_CLI, cases)
    refused = 0
    for case, plan in zip(cases, plans):
        want = _restated(*case)
        got_bytes = C.c_int64(-1)
        rc = N.lib().ftk_lightglue_adaptive_workspace_bytes(*case, C.byref(got_bytes))
        if want is None:
            refused += 1
            assert plan == {"refused": "layer"} and rc == -1, case
            continue
        assert plan.pop("refused") == "none" and {k: int(v) for k, v in plan.items()} == want, case
        assert rc == 0 and got_bytes.value == want["bytes"] == N.lightglue_adaptive_workspace_bytes(*case), case
        assert all(want[k] % 16 == 0 for k in want if k.startswith("off_")) and want["decide_threads"] * 16 >= max(case[:2])
    assert 0 < refused < len(cases)


def test_header_library_and_binding_agree():
    from feature_tracker_amd import _native as N
    header = A.header_library_and_binding_agree(("FTK_LIGHTGLUE_MAX_LAYERS", "FTK_LIGHTGLUE_STATE_WORDS"), ENTRIES)
    plan = open(os.path.join(A.ROOT, "feature_tracker_amd", "csrc", "lightglue_adaptive_plan.h")).read()
    assert all(getattr(N.lib(), name).argtypes is not None for name in ENTRIES)
    assert re.search(r"kAdaptiveMaxLayers = %d;" % N.FTK_LIGHTGLUE_MAX_LAYERS, plan) and re.search(r"kAdaptiveStateWords = %d " % N.FTK_LIGHTGLUE_STATE_WORDS, plan)
    # the argument counts of the prototypes and of the bindings
    for name in ENTRIES:
        proto = re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)
        assert len(proto.split(",")) == len(getattr(N.lib(), name).argtypes), name


M, N_, DIM, HEADS, LAYERS = 6, 7, 16, 4, 3


def _confidence(w, gated=True):
    from feature_tracker_amd import device as D
    words = [w.t(name, "int32", 1) if gated else None for name in ("live0", "live1", "gate")]
    return D.lightglue_confidence_device(w.ctx, w.t("desc0", "float32", M, DIM), w.t("desc1", "float32", N_, DIM), w.t("token_w", "float32", DIM),
                                         w.t("token_b", "float32", 1), w.t("match_w", "float32", DIM), w.t("match_b", "float32", 1), *words,
                                         w.t("conf", "float32", M + N_), w.t("mt", "float32", M + N_))


def _workspace(w, m=M, n=N_, d=DIM):
    clip = lambda v, hi: min(max(v, 1), hi)  # noqa: E731
    m, n, d = clip(m, 4096), clip(n, 4096), clip(d, 1024)
    return w.t("workspace", "int64", 8 * (m + n) * d + (d + 1) * d + 4 * (m + n) + 64)  # (enough for every refused shape too)


def _layer(w, m=M, n=N_, d=DIM, h=HEADS):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    dh = d // h if isinstance(h, int) and h > 0 else 1
    return D.transformer_layer_adaptive_device(w.ctx, w.t("desc0", "float32", m, d), w.t("desc1", "float32", n, d), h, w.t("enc0", "float32", 2, m, dh),
                                               w.t("enc1", "float32", 2, n, dh), w.t("weights", "float32", N.transformer_layer_weight_offsets(d)[2]),
                                               w.t("live0", "int32", 1), w.t("live1", "int32", 1), w.t("gate", "int32", 1), _workspace(w, m, n, d))


def _half(w, which, m=M, n=N_, d=DIM, h=HEADS):
    dh = d // h
    return (w.t(f"{which} desc0", "float32", m, d), w.t(f"{which} desc1", "float32", n, d), w.t(f"{which} enc0", "float32", 2, m, dh),
            w.t(f"{which} enc1", "float32", 2, n, dh), w.t(f"{which} ind0", "int32", m), w.t(f"{which} ind1", "int32", n))


def _step(w, counts=True, layer=0, threshold=0.9, depth=0.95, width=0.99, least=0, alias=False):
    from feature_tracker_amd import device as D
    src = _half(w, "src")
    dst = src if alias else _half(w, "dst")
    return D.lightglue_adapt_step_device(w.ctx, HEADS, layer, w.t("conf", "float32", M + N_), w.t("mt", "float32", M + N_),
                                         w.t("count0", "int32", 1) if counts else None, w.t("count1", "int32", 1) if counts else None,
                                         w.t("state", "int32", 4), threshold, depth, width, least, src, dst, w.t("layers0", "int32", M),
                                         w.t("layers1", "int32", N_), _workspace(w))


def _finish(w, layers=LAYERS, min_score=-1.0e30):
    from feature_tracker_amd import device as D
    return D.lightglue_finish_device(w.ctx, w.t("desc0", "float32", M, DIM), w.t("desc1", "float32", N_, DIM), HEADS, w.t("head_w", "float32", layers, DIM + 1, DIM),
                                     w.t("head_b", "float32", layers, DIM + 1), w.t("state", "int32", 4), w.t("ind0", "int32", M), w.t("ind1", "int32", N_),
                                     min_score, _workspace(w), w.t("scores", "float32", M + 1, N_ + 1), w.t("match_index", "int32", M),
                                     w.t("status", "uint8", M), w.t("layers0", "int32", M), w.t("layers1", "int32", N_))


CALLS = {"ftk_lightglue_confidence_device": _confidence, "ftk_transformer_layer_adaptive_device": _layer, "ftk_lightglue_adapt_step_device": _step,
         "ftk_lightglue_finish_device": _finish}


@pytest.mark.parametrize("native", sorted(CALLS))
def test_entry_takes_no_pointer_of_an_unchecked_argument(monkeypatch, native):
    A.walk_call(monkeypatch, CALLS[native], [native])


@pytest.mark.parametrize("kind", ["dtype", "device", "shape"])
@pytest.mark.parametrize("native", sorted(CALLS))
def test_each_refused_tensor_stops_the_entry_before_the_library(monkeypatch, native, kind):
    """Every tensor argument of every entry in turn with a wrong dtype, on another device, and one element longer in its last dimension."""
    # (desc0 gives the call its sizes; the workspace has a least size, tested below)
    names = A.refusal_sweep(monkeypatch, CALLS[native], kind, reshape=A.one_column_more, skip=("desc0", "src desc0", "workspace"))
    assert len(names) == {"ftk_lightglue_confidence_device": 11, "ftk_transformer_layer_adaptive_device": 9, "ftk_lightglue_adapt_step_device": 20,
                          "ftk_lightglue_finish_device": 13}[native]


def test_other_refusals(monkeypatch):
    w = A.Walk(monkeypatch)
    for match, call, kw in (("FTK_TRANSFORMER_MAX_ROWS", _layer, dict(m=4097)), ("FTK_TRANSFORMER_MAX_ROWS", _layer, dict(n=0)),
                            ("must divide D", _layer, dict(h=3)), ("FTK_TRANSFORMER_MAX_HEAD_DIM", _layer, dict(d=6, h=2)),
                            ("num_heads must be", _layer, dict(h=0)), ("layer must be", _step, dict(layer=-1)), ("layer must be", _step, dict(layer=64)),
                            ("threshold must be", _step, dict(threshold=1.5)), ("depth_confidence must be", _step, dict(depth=1.5)),
                            ("width_confidence must be", _step, dict(width=float("nan"))), ("pruning_min_keypoints must be", _step, dict(least=-1)),
                            ("not in place", _step, dict(alias=True)), ("the number of layers must be", _finish, dict(layers=65)),
                            ("min_score must be a number", _finish, dict(min_score=float("nan")))):
        with pytest.raises(ValueError, match=match):
            call(w, **kw)
    assert w.lib.calls == [] and w.unchecked_reads == []
    short = A.Walk(monkeypatch)
    real_t = short.t
    short.t = lambda name, dtype, *shape: real_t(name, dtype, *((8,) if name == "workspace" else shape))
    for call in (_layer, _step, _finish):
        with pytest.raises(ValueError, match="^workspace must be"):
            call(short)
    assert short.lib.calls == []
    for call, kw in ((_confidence, dict(gated=False)), (_step, dict(counts=False)), (_step, dict(depth=-1, width=-1)), (_finish, dict(layers=64))):
        call(w, **kw)
    assert len(short.lib.calls) == 4  # (the later walk's recorder stands where the library stands)


def test_scalar_checks():
    from feature_tracker_amd import _device_lightglue_adaptive as A
    for bad in (1.5, float("nan"), True, "0.9"):
        with pytest.raises(ValueError, match="depth_confidence"):
            A.check_confidence("depth_confidence", bad)
    assert A.check_confidence("width_confidence", -1) == -1.0 and A.check_min_keypoints(0) == 0 and A.check_layer_index("layer", 63, 0) == 63
    for bad in (-1, 64, 1.0, True):
        with pytest.raises(ValueError, match="layer"):
            A.check_layer_index("layer", bad, 0)
    assert A.stop_threshold(0, 9) == pytest.approx(0.9) and A.stop_threshold(8, 9) == pytest.approx(0.8 + 0.1 * 2.718281828 ** (-32 / 9))
