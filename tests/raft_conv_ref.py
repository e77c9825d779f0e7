"""ctypes binding of tests/raft_conv_ref.c — the scalar CPU restatement of the stock layers of RAFT's UpdateBlock and of the whole block
(DESIGN.md 5.14), compiled together with tests/sep_conv_gru_ref.c, whose GRU it calls for the middle.

TEST INFRASTRUCTURE ONLY: compiled on first use exactly as sep_conv_gru_ref.py does it (gcc -O3 -ffp-contract=off, plus -mfma where the
CPU has it) into a temporary directory; nothing under feature_tracker_amd/ may import it.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.flow_upsample_ref import same  # noqa: F401  (same: bit-identical, any NaN equals any NaN)
from tests.sep_conv_gru_ref import GATES
from tests.ref_build import FMA, STRICT, compile_ref

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRCS = [os.path.join(_HERE, "raft_conv_ref.c"), os.path.join(_HERE, "sep_conv_gru_ref.c")]

(CONTRACT, MUTANT_TAPS_FLIPPED, MUTANT_TAPS_TRANSPOSED, MUTANT_CLAMPED_PADDING, MUTANT_RELU_DROPPED, MUTANT_OUT_CONV_PARTS_EXCHANGED,
 MUTANT_FLOW_HEAD_ON_OLD_NET) = range(7)
MUTANTS = {"taps flipped": MUTANT_TAPS_FLIPPED, "ty and tx transposed": MUTANT_TAPS_TRANSPOSED, "clamped padding": MUTANT_CLAMPED_PADDING,
           "relu dropped": MUTANT_RELU_DROPPED, "temp_flow before temp_correlation": MUTANT_OUT_CONV_PARTS_EXCHANGED,
           "flow head fed the old net": MUTANT_FLOW_HEAD_ON_OLD_NET}
# the reference module's nine Conv2d layers, in the order rc_update_block takes them
LAYERS = ("motion_encoder.correlation_conv.0", "motion_encoder.correlation_conv.2", "motion_encoder.flow_conv.0", "motion_encoder.flow_conv.2",
          "motion_encoder.out_conv.0", "flow_head.conv1", "flow_head.conv2", "mask.0", "mask.2")


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("raft_conv_ref", _SRCS, flags=STRICT + FMA)  # -mfma where the CPU has it: fmaf as one instruction (see above)
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    l.rc_conv2d.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, f32, i32, i32, i32, i32, vp]
    l.rc_conv2d.restype = i32
    l.rc_update_block.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    l.rc_update_block.restype = i32
    return l


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)


def conv2d(parts, weight, bias, relu: bool, scale: float = 1.0, variant: int = CONTRACT):
    """parts: one float32 array [B, C, H, W] or a sequence of them; weight [Cout, Cin, ks, ks]; bias [Cout] -> [B, Cout, H, W]."""
    parts = [parts] if isinstance(parts, np.ndarray) else list(parts)
    parts = [_f32(p) for p in parts]
    weight, bias = _f32(weight), _f32(bias)
    B, _, H, W = parts[0].shape
    Cout, Cin, ks, ks2 = weight.shape
    assert ks == ks2 and bias.shape == (Cout,) and sum(p.shape[1] for p in parts) == Cin, (weight.shape, bias.shape, [p.shape for p in parts])
    assert all(p.shape == (B, p.shape[1], H, W) for p in parts)
    ptrs = (C.c_void_p * len(parts))(*[p.ctypes.data for p in parts])
    channels = (C.c_int32 * len(parts))(*[p.shape[1] for p in parts])
    out = np.empty((B, Cout, H, W), np.float32)
    rc = lib().rc_conv2d(ptrs, channels, len(parts), _p(weight), _p(bias), Cout, ks, int(bool(relu)), float(scale), B, H, W, int(variant), _p(out))
    assert rc == 0, rc
    return out


def weights_of(state, prefix=""):
    """Every tensor of a state dict of the reference's UpdateBlock (torch tensors or arrays) under ``prefix``, as float32 numpy arrays."""
    out = {}
    for layer in LAYERS + tuple(f"gru.conv_{g}" for g in GATES):
        for kind in ("weight", "bias"):
            out[f"{layer}.{kind}"] = _f32(state[f"{prefix}{layer}.{kind}"])
    return out


def update_block(net, inp, correlation, flow, state, variant: int = CONTRACT):
    """update_block.py:61-67 on float32 arrays; state: weights_of(...).  Returns (new_net, mask, delta_flow, features): the module's three
    outputs and the motion encoder's ``out`` (before its cat with flow)."""
    net, inp, correlation, flow = (_f32(t) for t in (net, inp, correlation, flow))
    w = {k: state[k + ".weight"] for k in LAYERS}
    B, Cnet, H, W = net.shape
    gru_w = [state[f"gru.conv_{g}.weight"] for g in GATES]
    gru_b = [state[f"gru.conv_{g}.bias"] for g in GATES]
    gru_ks = max(gru_w[0].shape[2:])
    motion_out = w["motion_encoder.out_conv.0"].shape[0] + 2
    sizes = [Cnet, inp.shape[1], correlation.shape[1], w[LAYERS[0]].shape[0], w[LAYERS[1]].shape[0], w[LAYERS[2]].shape[0], w[LAYERS[3]].shape[0], motion_out,
             w["flow_head.conv1"].shape[0], w["mask.0"].shape[0], w["mask.2"].shape[0], gru_ks, B, H, W]
    # the shapes the C side assumes
    expect = {LAYERS[0]: (sizes[3], sizes[2], 1), LAYERS[1]: (sizes[4], sizes[3], 3), LAYERS[2]: (sizes[5], 2, 7), LAYERS[3]: (sizes[6], sizes[5], 3),
              LAYERS[4]: (motion_out - 2, sizes[4] + sizes[6], 3), LAYERS[5]: (sizes[8], Cnet, 3), LAYERS[6]: (2, sizes[8], 3), LAYERS[7]: (sizes[9], Cnet, 3),
              LAYERS[8]: (sizes[10], sizes[9], 1)}
    for layer, (M, Cin, ks) in expect.items():
        assert w[layer].shape == (M, Cin, ks, ks) and state[layer + ".bias"].shape == (M,), (layer, w[layer].shape)
    Cx = inp.shape[1] + motion_out
    for k, wk in enumerate(gru_w):
        assert wk.shape == ((Cnet, Cx + Cnet, 1, gru_ks) if k < 3 else (Cnet, Cx + Cnet, gru_ks, 1)) and gru_b[k].shape == (Cnet,), (k, wk.shape)
    assert inp.shape == (B, inp.shape[1], H, W) and correlation.shape == (B, sizes[2], H, W) and flow.shape == (B, 2, H, W)
    conv_w = (C.c_void_p * 9)(*[w[k].ctypes.data for k in LAYERS])
    conv_b = (C.c_void_p * 9)(*[state[k + ".bias"].ctypes.data for k in LAYERS])
    gw = (C.c_void_p * 6)(*[a.ctypes.data for a in gru_w])
    gb = (C.c_void_p * 6)(*[a.ctypes.data for a in gru_b])
    new_net = np.empty_like(net)
    mask = np.empty((B, sizes[10], H, W), np.float32)
    delta_flow = np.empty((B, 2, H, W), np.float32)
    features = np.empty((B, motion_out - 2, H, W), np.float32)
    rc = lib().rc_update_block(_p(net), _p(inp), _p(correlation), _p(flow), conv_w, conv_b, gw, gb, (C.c_int32 * 15)(*sizes), int(variant), _p(new_net),
                               _p(mask), _p(delta_flow), _p(features))
    assert rc == 0, rc
    return new_net, mask, delta_flow, features
