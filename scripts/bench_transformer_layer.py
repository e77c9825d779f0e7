"""Time of one TransformerLayer and of LightGlue with 9 layers at D = 256, h = 4, M = N = 300, 1 024 and 2 048, against the same steps in
stock torch ops on the same device (``F.linear``, ``F.scaled_dot_product_attention``, ``F.layer_norm``, ``F.gelu``; DESIGN.md 5.24 and
6.18).  The torch composition rounds differently (and may pick any attention kernel) and is a yardstick for time only.  Calls are
interleaved in one process and the medians of 30 device-synchronised wall times are reported, one JSON line per shape (appended to --out,
default profiles/transformer_layer_bench.jsonl).  No time is asserted anywhere.  Not measured: captured graphs, counts below the row
count, other D or h."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_scenes import DIM, HEADS, LAYERS, SIZES, lightglue_inputs, state_dict  # noqa: E402
from scripts.benchlib import interleaved, parser, us_fields, write_rows  # noqa: E402


def torch_layer(torch, sd, i, x0, x1, e0, e1):
    F = torch.nn.functional
    p = f"transformers.{i}."
    lin = lambda name, x: F.linear(x, sd[p + name + ".weight"], sd[p + name + ".bias"])  # noqa: E731
    heads = lambda t: t.unflatten(-1, (HEADS, -1)).transpose(0, 1)  # noqa: E731

    def rot(t, enc):
        x1_, x2_ = t.unflatten(-1, (-1, 2)).unbind(dim=-1)
        return t * enc[0] + torch.stack((-x2_, x1_), dim=-1).flatten(start_dim=-2) * enc[1]

    def ffn(block, x, msg):
        hid = lin(block + ".ffn.0", torch.cat([x, msg], -1))
        hid = F.gelu(F.layer_norm(hid, (hid.shape[-1],), sd[p + block + ".ffn.1.weight"], sd[p + block + ".ffn.1.bias"]))
        return x + lin(block + ".ffn.3", hid)

    def self_block(x, enc):
        qkv = lin("self_attn.Wqkv", x).unflatten(-1, (HEADS, -1, 3)).transpose(0, 1)
        ctx = F.scaled_dot_product_attention(rot(qkv[..., 0], enc), rot(qkv[..., 1], enc), qkv[..., 2])
        return ffn("self_attn", x, lin("self_attn.out_proj", ctx.transpose(0, 1).flatten(start_dim=-2)))

    x0, x1 = self_block(x0, e0.unsqueeze(1)), self_block(x1, e1.unsqueeze(1))
    qk0, qk1, v0, v1 = heads(lin("cross_attn.to_qk", x0)), heads(lin("cross_attn.to_qk", x1)), heads(lin("cross_attn.to_v", x0)), heads(lin("cross_attn.to_v", x1))
    m0 = F.scaled_dot_product_attention(qk0, qk1, v1).transpose(0, 1).flatten(start_dim=-2)
    m1 = F.scaled_dot_product_attention(qk1, qk0, v0).transpose(0, 1).flatten(start_dim=-2)
    return ffn("cross_attn", x0, lin("cross_attn.to_out", m0)), ffn("cross_attn", x1, lin("cross_attn.to_out", m1))


def rows(args, torch):
    import feature_tracker_amd as F

    rng = np.random.default_rng(1)
    sd = state_dict(torch, rng)
    lg = F.LightGlue.from_state_dict(sd, num_heads=HEADS)
    size = (640.0, 480.0)
    for n in SIZES:
        a, b, kp0, kp1 = lightglue_inputs(torch, rng, n, size)
        e0, e1 = F.rotary_encoding(kp0, size, sd["posenc.Wr.weight"]), F.rotary_encoding(kp1, size, sd["posenc.Wr.weight"])

        def torch_all():
            x0, x1 = a, b
            for i in range(LAYERS):
                x0, x1 = torch_layer(torch, sd, i, x0, x1, e0, e1)
            return x0, x1

        calls = {"layer": lambda: lg.layers[0](a, b, e0, e1), "torch_layer": lambda: torch_layer(torch, sd, 0, a, b, e0, e1),
                 "lightglue_scores": lambda: lg.scores(kp0, kp1, a, b, size, size), "torch_nine_layers": torch_all}
        times = interleaved(torch, calls, args.repeats, args.warmup)
        got, want = lg.layers[0](a, b, e0, e1), torch_layer(torch, sd, 0, a, b, e0, e1)
        row = {"bench": "transformer_layer", "rows": n, "dim": DIM, "heads": HEADS, "layers": LAYERS,
               "max_abs_difference_to_torch": float(max((got[0] - want[0]).abs().max().item(), (got[1] - want[1]).abs().max().item()))}
        for label in calls:
            us_fields(row, label, times[label])
        yield row


def main():
    args = parser("--repeats", 30, 5, os.path.join(ROOT, "profiles", "transformer_layer_bench.jsonl")).parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=True, extra={"device": torch.cuda.get_device_name(0)})


if __name__ == "__main__":
    main()
