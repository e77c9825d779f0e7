#!/usr/bin/env python3
"""Writes tests/golden/raft/raft_model_small.npz (a directory of its own: every .npz directly under tests/golden/ is an oracle fixture
that tests/test_oracle_cpu.py replays): a state dict, an image pair and the float32 predictions of the reference's own ``Raft``
(src/nn_optical_flow_tracker/raft/model.py) on torch CPU, for tests/test_raft_encoder_cpu.py.

    python tests/golden/make_raft_model.py --reference <checkout of Horizon1026/Feature_Tracker>

The reference's module is loaded by path at run time (its directory goes on sys.path for its own ``from encoder import *``); nothing of
it is copied.  Needs the checkout, so no test imports this script: the suite reads the committed .npz.

The module is put in eval mode; its default initialisation (seeded) and randomised BatchNorm running statistics (the defaults, mean 0 and
variance 1, would let a wrong fold pass) are rounded to multiples of 2^-8, and that state dict is loaded back into it before the forward
pass.  Keys: ``state/<name>`` for every entry of ``state_dict()``, ``ref_image``, ``cur_image`` (whole numbers in 0 .. 255),
``prediction_<i>``, and ``sizes`` (the constructor's thirteen arguments, then B, H, W).
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

# tests/test_raft_encoder_cpu.py's tiny model on a 16 x 24 pair: one correlation level of radius 1 (a 2 x 3 feature map has no second level)
SIZES = dict(in_channels=1, hidden_channels=4, feature_channels=8, context_channels=4, correlation_pyramid_levels=1, correlation_radius=1,
             correlation_hidden_channels=4, correlation_out_channels=4, flow_hidden_channels=4, flow_out_channels=4, motion_out_channels=6,
             mask_hidden_channels=4, max_iterations=2)
B, H, W = 1, 16, 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "raft", "raft_model_small.npz"))
    args = ap.parse_args()
    raft_dir = os.path.join(args.reference, "src", "nn_optical_flow_tracker", "raft")
    sys.path.insert(0, raft_dir)
    spec = importlib.util.spec_from_file_location("reference_raft_model", os.path.join(raft_dir, "model.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)

    torch.manual_seed(30)
    model = module.Raft(**SIZES).eval()
    g = torch.Generator().manual_seed(31)
    state = {}
    for k, v in model.state_dict().items():
        if k.endswith("running_mean"):
            v = 0.5 * torch.randn(v.shape, generator=g)
        elif k.endswith("running_var"):
            v = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith("num_batches_tracked"):
            state[k] = v
            continue
        elif ".bn" in k or ".shortcut.1." in k:  # gamma, beta
            v = (0.5 + torch.rand(v.shape, generator=g)) if k.endswith("weight") else 0.3 * torch.randn(v.shape, generator=g)
        state[k] = torch.round(v * 256.0) / 256.0
    model.load_state_dict(state)
    ref_image = torch.floor(256.0 * torch.rand(B, 1, H, W, generator=g)).clamp(0, 255)
    cur_image = torch.floor(256.0 * torch.rand(B, 1, H, W, generator=g)).clamp(0, 255)
    with torch.no_grad():
        predictions = model(ref_image, cur_image)
    arrays = {"state/" + k: v.numpy() for k, v in model.state_dict().items()}
    arrays.update(ref_image=ref_image.numpy(), cur_image=cur_image.numpy(), sizes=np.int32(list(SIZES.values()) + [B, H, W]))
    arrays.update({f"prediction_{i}": p.numpy() for i, p in enumerate(predictions)})
    assert len(predictions) == SIZES["max_iterations"] and all(p.dtype == torch.float32 and p.shape == (B, 2, H, W) for p in predictions)
    np.savez_compressed(args.out, **arrays)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
