#!/usr/bin/env python3
"""Writes tests/golden/raft/raft_update_block_small.npz (a directory of its own: every .npz directly under tests/golden/ is an oracle
fixture that tests/test_oracle_cpu.py replays): a state dict, four inputs and the three float32 outputs of the reference's own
``UpdateBlock`` (src/nn_optical_flow_tracker/raft/update_block.py) on torch CPU, for tests/test_update_block_cpu.py.

    python tests/golden/make_raft_update_block.py --reference <checkout of Horizon1026/Feature_Tracker>

The reference's module is loaded by path at run time (its directory goes on sys.path for its own ``from gru import *``); nothing of it
is copied.  Needs the checkout, so no test imports this script: the suite reads the committed .npz.

The module keeps its default initialisation (seeded) rounded to multiples of 2^-8, and that state dict is loaded back into it before
the forward pass: the low mantissa bytes of the weights are zero and the archive compresses under 100 KB (the 576-channel mask, which
is full-entropy float32, is more than half of it).  Keys: ``state/<name>`` for every entry of ``state_dict()``, ``net``, ``inp``,
``correlation``, ``flow``, ``new_net``, ``mask``, ``delta_flow``, and ``sizes`` (the constructor's nine arguments, then B, H, W).
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

# tests/test_update_block_cpu.py's first case, on a 3 x 4 grid
SIZES = dict(net_in_channels=16, inp_in_channels=3, corr_in_channels=18, corr_hidden_channels=16, corr_out_channels=12, flow_hidden_channels=8,
             flow_out_channels=4, motion_out_channels=10, mask_hidden_channels=8)
B, H, W = 2, 3, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "raft", "raft_update_block_small.npz"))
    args = ap.parse_args()
    raft_dir = os.path.join(args.reference, "src", "nn_optical_flow_tracker", "raft")
    sys.path.insert(0, raft_dir)
    spec = importlib.util.spec_from_file_location("reference_update_block", os.path.join(raft_dir, "update_block.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)

    torch.manual_seed(20)
    block = module.UpdateBlock(**SIZES).eval()
    state = {k: torch.round(v * 256.0) / 256.0 for k, v in block.state_dict().items()}
    block.load_state_dict(state)
    g = torch.Generator().manual_seed(21)
    net = torch.tanh(torch.randn(B, SIZES["net_in_channels"], H, W, generator=g))
    inp = torch.relu(torch.randn(B, SIZES["inp_in_channels"], H, W, generator=g))
    correlation = torch.randn(B, SIZES["corr_in_channels"], H, W, generator=g)
    flow = 2.0 * torch.randn(B, 2, H, W, generator=g)
    with torch.no_grad():
        new_net, mask, delta_flow = block(net, inp, correlation, flow)
    arrays = {"state/" + k: v.numpy() for k, v in block.state_dict().items()}
    arrays.update(net=net.numpy(), inp=inp.numpy(), correlation=correlation.numpy(), flow=flow.numpy(), new_net=new_net.numpy(), mask=mask.numpy(),
                  delta_flow=delta_flow.numpy(), sizes=np.int32(list(SIZES.values()) + [B, H, W]))
    assert all(a.dtype == np.float32 for k, a in arrays.items() if k != "sizes")
    np.savez_compressed(args.out, **arrays)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
