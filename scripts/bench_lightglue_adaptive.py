"""Time of ``LightGlue.match_adaptive`` at D = 256, h = 4, nine layers, M = N = 300, 1 024 and 2 048, with seeded
weights steered as in the tests: the token heads have no weights and a bias of -30 (never confident) or +30 (confident), the
matchability head of the pruning layer gets the bias that puts the median row on the bar.  Per size, in one process and interleaved:

  * ``match``: ``LightGlue.match``, full depth and width, the path without any of the adaptive steps;
  * ``adaptive_full``: ``match_adaptive`` that never stops and keeps every row: the cost of the per-layer steps and of the gate;
  * ``adaptive_stop3``: a stop after 3 of the 9 layers (the other 6 are launched and return at their gate);
  * ``adaptive_prune_half``: about half of each side pruned after layer 1, no stop;
  * ``layer_open`` / ``layer_gated``: ``transformer_layer_adaptive_device`` alone with its gate at 0 and at 1.

Medians of 30 device-synchronised wall times, one JSON line per size (appended to --out, default
profiles/lightglue_adaptive_bench.jsonl), with the stop layer and live counts each pass ended with.  No time is asserted anywhere.  With
random weights nothing is claimed about matching quality or typical stop layers."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_scenes import DIM, HEADS, LAYERS, SIZES, lightglue_inputs, state_dict  # noqa: E402
from scripts.benchlib import interleaved, parser, us_fields, write_rows  # noqa: E402


def adaptive_state_dict(torch, base, rng, token_bias, match_bias):
    """``base`` with token_confidence.{i} (no weights, the given biases) and log_assignment.{i} of every layer."""
    sd, d = dict(base), DIM
    for i in range(LAYERS):
        head = f"log_assignment.{i}."
        if i < LAYERS - 1:
            sd[head + "final_proj.weight"] = torch.from_numpy((np.eye(d) + rng.standard_normal((d, d)) / np.sqrt(d) * 0.5).astype(np.float32)).cuda()
            sd[head + "final_proj.bias"] = torch.zeros(d).cuda()
            sd[head + "matchability.weight"] = torch.from_numpy((rng.standard_normal((1, d)) / np.sqrt(d)).astype(np.float32)).cuda()
            sd[f"token_confidence.{i}.token.0.weight"] = torch.zeros(1, d).cuda()
            sd[f"token_confidence.{i}.token.0.bias"] = torch.tensor([token_bias[i]], dtype=torch.float32).cuda()
        sd[head + "matchability.bias"] = torch.tensor([match_bias[i]], dtype=torch.float32).cuda()
    return sd


def rows(args, torch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D

    rng = np.random.default_rng(1)
    base = state_dict(torch, rng)
    never, keep = [-30.0] * LAYERS, [30.0] * LAYERS
    head_rng = lambda: np.random.default_rng(2)  # noqa: E731  (the same heads in every state dict)
    sd_full = adaptive_state_dict(torch, base, head_rng(), never, keep)
    sd_stop = adaptive_state_dict(torch, base, head_rng(), [-30.0, -30.0] + [30.0] * (LAYERS - 2), keep)
    lg_plain = F.LightGlue.from_state_dict(sd_full, num_heads=HEADS)
    lg_full = F.LightGlue.from_state_dict(sd_full, num_heads=HEADS, depth_confidence=0.95, width_confidence=0.99, pruning_min_keypoints=0)
    lg_stop = F.LightGlue.from_state_dict(sd_stop, num_heads=HEADS, depth_confidence=0.95, width_confidence=0.99, pruning_min_keypoints=0)
    size = (640.0, 480.0)
    for n in SIZES:
        a, b, kp0, kp1 = lightglue_inputs(torch, rng, n, size)
        e0, e1 = F.rotary_encoding(kp0, size, base["posenc.Wr.weight"]), F.rotary_encoding(kp1, size, base["posenc.Wr.weight"])
        # the matchability z of the rows after layers 0 and 1: its median goes on the bar logit(1 - 0.9) = -2.2 at layer 1
        x0, x1 = a, b
        for i in range(2):
            x0, x1 = lg_plain.layers[i](x0, x1, e0, e1)
        z = torch.cat([x0, x1]) @ sd_full["log_assignment.1.matchability.weight"][0]
        bias = keep[:1] + [float(-2.2 - z.median().item())] + keep[2:]
        sd_prune = adaptive_state_dict(torch, base, head_rng(), never, bias)
        lg_prune = F.LightGlue.from_state_dict(sd_prune, num_heads=HEADS, depth_confidence=-1, width_confidence=0.9, pruning_min_keypoints=0)
        # the layer alone, in place on copies, with the pass's own workspace
        ctx = F.default_context()
        ws = torch.empty(-(-N.lightglue_adaptive_workspace_bytes(n, n, DIM, HEADS) // 8), dtype=torch.int64, device="cuda")
        w0 = next(iter(lg_plain.layers[0]._packed.values()))
        c0, c1 = a.clone(), b.clone()
        live = torch.tensor([n], dtype=torch.int32, device="cuda")
        gates = {label: torch.tensor([value], dtype=torch.int32, device="cuda") for label, value in (("layer_open", 0), ("layer_gated", 1))}
        layer = lambda gate: D.transformer_layer_adaptive_device(ctx, c0, c1, HEADS, e0, e1, w0, live, live, gate, ws)  # noqa: E731
        calls = {"match": lambda: lg_plain.match(kp0, kp1, a, b, size, size),
                 "adaptive_full": lambda: lg_full.match_adaptive(kp0, kp1, a, b, size, size),
                 "adaptive_stop3": lambda: lg_stop.match_adaptive(kp0, kp1, a, b, size, size),
                 "adaptive_prune_half": lambda: lg_prune.match_adaptive(kp0, kp1, a, b, size, size),
                 "layer_open": lambda: layer(gates["layer_open"]), "layer_gated": lambda: layer(gates["layer_gated"])}
        times = interleaved(torch, calls, args.repeats, args.warmup)
        row = {"bench": "lightglue_adaptive", "rows": n, "dim": DIM, "heads": HEADS, "layers": LAYERS}
        for label, lg in (("adaptive_full", lg_full), ("adaptive_stop3", lg_stop), ("adaptive_prune_half", lg_prune)):
            r = lg.match_adaptive(kp0, kp1, a, b, size, size)
            torch.cuda.synchronize()
            row[f"{label}_stop_layer"], row[f"{label}_live"] = int(r.stop_layer.item()), [int(r.live0.item()), int(r.live1.item())]
        full = lg_full.match_adaptive(kp0, kp1, a, b, size, size)
        plain = lg_plain.match(kp0, kp1, a, b, size, size)
        row["adaptive_full_equals_match"] = bool(torch.equal(full.match_index, plain[1]) and torch.equal(full.scores, plain[0]))
        for label in calls:
            us_fields(row, label, times[label])
        yield row


def main():
    args = parser("--repeats", 30, 5, os.path.join(ROOT, "profiles", "lightglue_adaptive_bench.jsonl")).parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=True, extra={"device": torch.cuda.get_device_name(0)})


if __name__ == "__main__":
    main()
