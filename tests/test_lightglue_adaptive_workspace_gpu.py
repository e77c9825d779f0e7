"""The adaptive pass held to the sizes it declares, as tests/test_transformer_workspace_gpu.py holds the layer: the four
device entries called directly on guarded memory (tests/guarded.py), the workspace exactly
``ceil(ftk_lightglue_adaptive_workspace_bytes / 8)`` int64 words and every other buffer a payload of exactly its shape; twice on fresh
arenas, all payloads 0x00 and all 0xFF, both results equal to the scalar restatement bit for bit; no guard band written; the weights
come back bit for bit."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import guarded as G
from tests import lightglue_adaptive_ref as R

pytestmark = pytest.mark.gpu

SHAPES = (R.SHAPES[1], R.SHAPES[2], R.SHAPES[4])  # a partial tile; a key tile and a row tile crossed by the pruning; the non-vector bodies
HALF = ("desc0", "desc1", "enc0", "enc1", "ind0", "ind1")


def _run(ftk, shape, case, depth, width, counts, fill):
    import torch
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    from feature_tracker_amd._device_lightglue_adaptive import stop_threshold
    m, n, d, h, _ = shape
    a, b, e0, e1, sd = case
    L, dh = R.N_LAYERS, d // h
    lg = ftk.LightGlue.from_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, num_heads=h, depth_confidence=depth, width_confidence=width,
                                       pruning_min_keypoints=0)
    token_w, token_b, head_w, head_b = (t.numpy() for t in lg._adaptive[3:])
    n0, n1 = (m, n) if counts is None else counts
    inputs = dict(token_w=token_w, token_b=token_b, head_w=head_w, head_b=head_b)
    inputs.update({f"layer{i}": next(iter(lg.layers[i]._packed.values())).numpy() for i in range(L)})
    start = dict(a_desc0=a, a_desc1=b, a_enc0=e0, a_enc1=e1, a_ind0=np.arange(m, dtype=np.int32), a_ind1=np.arange(n, dtype=np.int32),
                 state=np.array([n0, n1, 0, L - 1], np.int32), layers0=np.zeros(m, np.int32), layers1=np.zeros(n, np.int32))
    if counts is not None:
        inputs.update(count0=np.array([n0], np.int32), count1=np.array([n1], np.int32))
    specs = [(name, str(v.dtype), v.shape, 0) for name, v in list(inputs.items()) + list(start.items())]
    specs += [(f"b_{k}", str(start[f"a_{k}"].dtype), start[f"a_{k}"].shape, 0) for k in HALF]
    specs += [("conf", "float32", (m + n,), 0), ("mt", "float32", (m + n,), 0), ("scores", "float32", (m + 1, n + 1), 0), ("match_index", "int32", (m,), 0),
              ("status", "uint8", (m,), 0), ("workspace", "int64", (-(-N.lightglue_adaptive_workspace_bytes(m, n, d, h) // 8),), 0)]
    arena = G.Arena(specs, "cuda", fill=fill)
    for name, array in list(inputs.items()) + list(start.items()):
        arena.put(name, array)
    ctx, t = ftk.default_context(), arena
    halves = [tuple(t[f"{p}_{k}"] for k in HALF) for p in ("a", "b")]
    state = t["state"]
    live0, live1, gate = state[0:1], state[1:2], state[2:3]
    c0, c1 = (t["count0"], t["count1"]) if counts is not None else (None, None)
    for i in range(L):
        cur, nxt = halves[i % 2], halves[(i + 1) % 2]
        D.transformer_layer_adaptive_device(ctx, cur[0], cur[1], h, cur[2], cur[3], t[f"layer{i}"], live0, live1, gate, t["workspace"])
        if i < L - 1:
            D.lightglue_confidence_device(ctx, cur[0], cur[1], t["token_w"][i], t["token_b"][i:i + 1], t["head_w"][i, d], t["head_b"][i, d:d + 1], live0, live1,
                                          gate, t["conf"], t["mt"])
            D.lightglue_adapt_step_device(ctx, h, i, t["conf"], t["mt"], c0, c1, state, stop_threshold(i, L), float(depth), float(width), 0, cur, nxt,
                                          t["layers0"], t["layers1"], t["workspace"])
    last = halves[(L - 1) % 2]
    D.lightglue_finish_device(ctx, last[0], last[1], h, t["head_w"], t["head_b"], state, last[4], last[5], -1.0e30, t["workspace"], t["scores"],
                              t["match_index"], t["status"], t["layers0"], t["layers1"])
    torch.cuda.synchronize()
    host = arena.check()
    for name, array in inputs.items():
        assert arena.payload_bytes(name, host).tobytes() == np.ascontiguousarray(array).tobytes(), f"the pass changed its input {name}"
    f = {k: t[k].cpu().numpy() for k in ("match_index", "status", "scores", "state", "layers0", "layers1")}
    return SimpleNamespace(match_index=f["match_index"], status=f["status"], scores=f["scores"], ind0=last[4].cpu().numpy(), ind1=last[5].cpu().numpy(),
                           live0=int(f["state"][0]), live1=int(f["state"][1]), stop_layer=int(f["state"][3]), layers0=f["layers0"], layers1=f["layers1"])


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(str(v) for v in s[:4]) for s in SHAPES])
def test_the_pass_in_its_declared_bytes(ftk, shape):
    from feature_tracker_amd import _native as N
    m, n, d, h, _ = shape
    declared = C.c_int64()
    assert N.lib().ftk_lightglue_adaptive_workspace_bytes(m, n, d, h, C.byref(declared)) == 0
    assert declared.value == N.lightglue_adaptive_workspace_bytes(m, n, d, h) and declared.value % 16 == 0
    pruning, depth, width = R.prune_case(shape, True)
    kwargs, stop_depth, stop_width = R.STOP_AT_1
    stopping = R.case(shape, **kwargs)
    mid = ((2 * m + 2) // 3, (3 * n + 3) // 4)
    for case, dc, wc, counts in ((pruning, depth, width, None), (pruning, depth, width, mid), (stopping, stop_depth, stop_width, mid)):
        a, b, e0, e1, sd = case
        want = R.run(a, b, h, e0, e1, sd, R.N_LAYERS, dc, wc, 0, *(counts or (None, None)))
        for fill in (G.ZEROS, G.ONES):
            got = _run(ftk, shape, case, dc, wc, counts, fill)
            assert R.same_outputs(got, want), (shape, dc, wc, counts, hex(fill))
