"""Time of one TransformerLayer and of LightGlue with 9 layers at D = 256, h = 4, M = N = 300, 1 024 and 2 048, against the same steps in
stock torch ops on the same device (``F.linear``, ``F.scaled_dot_product_attention``, ``F.layer_norm``, ``F.gelu``; DESIGN.md 5.24 and
6.18).  The torch composition rounds differently (and may pick any attention kernel) and is a yardstick for time only.  Calls are
interleaved in one process and the medians of 30 device-synchronised wall times are reported, one JSON line per shape (appended to --out,
default profiles/transformer_layer_bench.jsonl).  No time is asserted anywhere.  Not measured: captured graphs, counts below the row
count, other D or h."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (300, 1024, 2048)
DIM, HEADS, LAYERS = 256, 4, 9


def timed(torch, fn, repeats, warmup):
    out = []
    for i in range(repeats + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(time.perf_counter() - t0)
    return out


def state_dict(torch, rng):
    sd, d = {}, DIM
    lin = lambda outs, ins: (torch.from_numpy((rng.standard_normal((outs, ins)) / np.sqrt(ins)).astype(np.float32)).cuda(),  # noqa: E731
                             torch.from_numpy((0.1 * rng.standard_normal(outs)).astype(np.float32)).cuda())
    for i in range(LAYERS):
        for block, names in (("self_attn", (("Wqkv", 3 * d, d), ("out_proj", d, d))), ("cross_attn", (("to_qk", d, d), ("to_v", d, d), ("to_out", d, d)))):
            for name, outs, ins in names + (("ffn.0", 2 * d, 2 * d), ("ffn.3", d, 2 * d)):
                sd[f"transformers.{i}.{block}.{name}.weight"], sd[f"transformers.{i}.{block}.{name}.bias"] = lin(outs, ins)
            sd[f"transformers.{i}.{block}.ffn.1.weight"], sd[f"transformers.{i}.{block}.ffn.1.bias"] = torch.ones(2 * d).cuda(), torch.zeros(2 * d).cuda()
    sd["posenc.Wr.weight"] = torch.from_numpy(rng.standard_normal((d // HEADS // 2, 2)).astype(np.float32)).cuda()
    head = f"log_assignment.{LAYERS - 1}."
    sd[head + "final_proj.weight"], sd[head + "final_proj.bias"] = lin(d, d)
    sd[head + "matchability.weight"], sd[head + "matchability.bias"] = lin(1, d)
    return sd


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transformer_layer_bench.jsonl"))
    args = ap.parse_args()
    import torch

    import feature_tracker_amd as F

    rng = np.random.default_rng(1)
    sd = state_dict(torch, rng)
    lg = F.LightGlue.from_state_dict(sd, num_heads=HEADS)
    size = (640.0, 480.0)
    rows = []
    for n in SIZES:
        x = rng.standard_normal((n, DIM))
        y = x[rng.permutation(n)] + 0.3 * rng.standard_normal((n, DIM))
        a = torch.from_numpy((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)).cuda()
        b = torch.from_numpy((y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)).cuda()
        kp0 = torch.from_numpy((rng.random((n, 2)) * np.array(size)).astype(np.float32)).cuda()
        kp1 = torch.from_numpy((rng.random((n, 2)) * np.array(size)).astype(np.float32)).cuda()
        e0, e1 = F.rotary_encoding(kp0, size, sd["posenc.Wr.weight"]), F.rotary_encoding(kp1, size, sd["posenc.Wr.weight"])

        def torch_all():
            x0, x1 = a, b
            for i in range(LAYERS):
                x0, x1 = torch_layer(torch, sd, i, x0, x1, e0, e1)
            return x0, x1

        calls = {"layer": lambda: lg.layers[0](a, b, e0, e1), "torch_layer": lambda: torch_layer(torch, sd, 0, a, b, e0, e1),
                 "lightglue_scores": lambda: lg.scores(kp0, kp1, a, b, size, size), "torch_nine_layers": torch_all}
        times = {label: [] for label in calls}
        for _ in range(3):  # interleaved rounds
            for label, fn in calls.items():
                times[label] += timed(torch, fn, args.repeats // 3, args.warmup)
        got, want = lg.layers[0](a, b, e0, e1), torch_layer(torch, sd, 0, a, b, e0, e1)
        row = {"bench": "transformer_layer", "rows": n, "dim": DIM, "heads": HEADS, "layers": LAYERS,
               "max_abs_difference_to_torch": float(max((got[0] - want[0]).abs().max().item(), (got[1] - want[1]).abs().max().item()))}
        for label in calls:
            row[f"{label}_us_median"] = round(1e6 * float(np.median(times[label])), 1)
            row[f"{label}_us_min"] = round(1e6 * float(np.min(times[label])), 1)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for row in rows:
        row["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
