#!/usr/bin/env python3
"""UpdateBlock (RAFT's refinement iteration without lookup and upsampling): time per call against the same
weights through the reference's composition (update_block.py:61-67) in stock torch ops on the same device, in the same run, and each
of the nine stock layers on its own against torch.nn.functional.conv2d + relu.

    python scripts/bench_update_block.py [--calls 100] [--warmup 10] [--out profiles/update_block_bench.jsonl]

Two shapes: the reference's model.py configuration (B 5 on the 8 x 8 grid of its 60 x 60 example images), and RAFT's usual one
(correlation 4 * 81 = 324 -> 256 -> 192, flow 2 -> 128 -> 64, motion 128, net and inp 128, mask hidden 256, 1 x 55 x 128).  Method as
in bench_sep_conv_gru.py: every call timed on its own with a pair of events after a warm-up, median / p10 / p90 of `calls` calls;
float32 on both sides.  One JSON line per shape:
  fused_ms, fused_ms_p10/p90          UpdateBlock: 13 launches
  torch_ms, torch_ms_p10/p90          the torch composition (its three cats and the 0.25 pass included, as in the reference)
  fused_speedup_vs_torch              torch over fused
  not_slower                          fused median <= torch median + (torch p90 - torch p10)
  max_abs_vs_torch                    largest |difference| of the three outputs (they differ in summation order)
  flop, fused_tflops                  2 * M * K * pixels over the nine layers and the GRU's twelve
  layers                              per layer: its shape, fused_ms, torch_ms (conv2d + relu [+ the 0.25 pass]), speedup, tflops
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import feature_tracker_amd as F  # noqa: E402
from feature_tracker_amd import _native, raft  # noqa: E402
from scripts.benchlib import event_times, ms_fields, parser, write_rows  # noqa: E402
from tests.test_update_block_cpu import GRU_KERNEL_SIZE, layer_shapes, make_inputs, make_state, torch_forward  # noqa: E402

# (name, (net, inp, corr, corr_hidden, corr_out, flow_hidden, flow_out, motion_out, mask_hidden), B, H, W)
SHAPES = [("model_py_60x60", (64, 128, 147, 64, 32, 32, 16, 32, 64), 5, 8, 8), ("raft_55x128", (128, 128, 324, 256, 192, 128, 64, 128, 256), 1, 55, 128)]
# layers with a ReLU after them; the mask head's last layer carries the 0.25
RELU = {"motion_encoder.correlation_conv.0", "motion_encoder.correlation_conv.2", "motion_encoder.flow_conv.0", "motion_encoder.flow_conv.2",
        "motion_encoder.out_conv.0", "flow_head.conv1", "mask.0"}


def rows(args, torch):
    dev = torch.device("cuda")
    Fn = torch.nn.functional
    for name, widths, B, H, W in SHAPES:
        state = {k: v.to(dev) for k, v in make_state(widths, 1).items()}
        block = F.UpdateBlock.from_state_dict(state, prefix="")
        inputs = [t.to(dev) for t in make_inputs(widths, B, H, W, 1)]
        ctx = raft._context(torch.cuda.current_device())
        pixels = B * H * W
        with torch.no_grad():
            fused = event_times(torch, [lambda: block(*inputs)], args.calls, args.warmup)
            stock = event_times(torch, [lambda: torch_forward(state, *inputs)], args.calls, args.warmup)
            diff = max(float((a - b).abs().max()) for a, b in zip(block(*inputs), torch_forward(state, *inputs)[:3]))
            layers, flop = [], 0
            g = torch.Generator().manual_seed(7)
            for layer, (M, Cin, ks) in layer_shapes(*widths).items():
                x = torch.randn(B, Cin, H, W, generator=g).to(dev)
                w, b = state[layer + ".weight"], state[layer + ".bias"]
                relu, scale = layer in RELU, 0.25 if layer == "mask.2" else 1.0
                packed = block.motion_encoder._layers[layer[len("motion_encoder."):]] if layer.startswith("motion_encoder.") else block._layers[layer]

                def ours():
                    return raft._conv(ctx, [x], packed, relu, scale)

                def theirs():
                    y = Fn.conv2d(x, w, b, padding=ks // 2)
                    y = Fn.relu(y) if relu else y
                    return .25 * y if scale != 1.0 else y

                t_ours, t_theirs = event_times(torch, [ours], args.calls, args.warmup), event_times(torch, [theirs], args.calls, args.warmup)
                f = 2 * M * Cin * ks * ks * pixels
                flop += f
                entry = {"layer": layer, "out_channels": M, "in_channels": Cin, "kernel_size": ks}
                ms_fields(entry, "fused", t_ours)
                ms_fields(entry, "torch", t_theirs)
                entry.update({"speedup_vs_torch": round(t_theirs[0] / t_ours[0], 2), "fused_tflops": round(f / (t_ours[0] * 1e-3) / 1e12, 3),
                              "max_abs_vs_torch": float((ours() - theirs()).abs().max())})
                layers.append(entry)
        net, inp, motion_out = widths[0], widths[1], widths[7]
        flop += 2 * 2 * 3 * net * (inp + motion_out + net) * GRU_KERNEL_SIZE * pixels
        row = {"shape": name, "widths": list(widths), "B": B, "H": H, "W": W}
        ms_fields(row, "fused", fused, spread=True)
        ms_fields(row, "torch", stock, spread=True)
        row.update({"fused_speedup_vs_torch": round(stock[0] / fused[0], 2), "not_slower": bool(fused[0] <= stock[0] + (stock[2] - stock[1])),
                    "max_abs_vs_torch": diff, "flop": flop, "fused_tflops": round(flop / (fused[0] * 1e-3) / 1e12, 3), "layers": layers})
        yield row


def main():
    args = parser("--calls", 100, 10).parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=False, extra={"build": _native.build_info().get("source_hash", "?")})


if __name__ == "__main__":
    main()
