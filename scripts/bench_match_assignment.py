"""Time of MatchAssignment.assign and MatchAssignment.match at M = N = 300, 1 024 and 2 048 with D = 256, with weights and without,
against the same steps in stock torch ops: ``linear`` (projection and matchability), ``matmul``, ``log_softmax``
twice, ``logsigmoid`` and the assembly of the [M + 1, N + 1] tensor as upstream LightGlue writes it; for ``match`` the torch side adds
``max`` along both axes and the mutual check.  The torch composition rounds differently and is a yardstick for time only.  Calls are
interleaved in one process and the medians of 30 device-synchronised wall times are reported, one JSON line per shape and form (appended
to --out, default profiles/match_assignment_bench.jsonl).  No time is asserted anywhere."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.benchlib import interleaved, parser, us_fields, write_rows  # noqa: E402

SIZES = (300, 1024, 2048)
DIM = 256


def torch_assign(torch, a, b, weights, scale):
    F = torch.nn.functional
    m, n, d = a.shape[0], b.shape[0], a.shape[1]
    if weights is not None:
        fw, fb, mw, mb = weights
        md0, md1 = F.linear(a, fw, fb) / d ** .25, F.linear(b, fw, fb) / d ** .25
        z0, z1 = F.linear(a, mw, mb), F.linear(b, mw, mb)
    else:
        md0, md1 = a * scale, b * scale
    sim = md0 @ md1.t()
    scores0 = F.log_softmax(sim, 1)
    scores1 = F.log_softmax(sim.t().contiguous(), 1).t()
    scores = sim.new_full((m + 1, n + 1), 0.0 if weights is not None else float("-inf"))
    scores[m, n] = 0.0
    if weights is not None:
        scores[:m, :n] = scores0 + scores1 + F.logsigmoid(z0) + F.logsigmoid(z1).t()
        scores[:m, n] = F.logsigmoid(-z0.squeeze(-1))
        scores[m, :n] = F.logsigmoid(-z1.squeeze(-1))
    else:
        scores[:m, :n] = scores0 + scores1
    return scores


def torch_match(torch, scores, min_score):
    block = scores[:-1, :-1]
    best0, idx0 = block.max(1)
    idx1 = block.max(0).indices
    mutual = (idx1[idx0] == torch.arange(block.shape[0], device=block.device)) & (best0 > min_score)
    return torch.where(mutual, idx0, torch.full_like(idx0, -1)).int(), mutual.to(torch.uint8)


def rows(args, torch):
    import feature_tracker_amd as F

    rng = np.random.default_rng(1)
    fw = torch.from_numpy((np.eye(DIM) + 0.5 * rng.standard_normal((DIM, DIM)) / np.sqrt(DIM)).astype(np.float32)).cuda()
    fb = torch.from_numpy((0.1 * rng.standard_normal(DIM)).astype(np.float32)).cuda()
    mw = torch.from_numpy((rng.standard_normal((1, DIM)) / np.sqrt(DIM)).astype(np.float32)).cuda()
    mb = torch.from_numpy((0.5 * rng.standard_normal(1)).astype(np.float32)).cuda()
    sd = {"log_assignment.8.final_proj.weight": fw, "log_assignment.8.final_proj.bias": fb, "log_assignment.8.matchability.weight": mw,
          "log_assignment.8.matchability.bias": mb}
    heads = {True: F.MatchAssignment.from_state_dict(sd), False: F.MatchAssignment.without_weights(DIM)}
    for size in SIZES:
        x = rng.standard_normal((size, DIM))
        y = x[rng.permutation(size)] + 0.3 * rng.standard_normal((size, DIM))
        a = torch.from_numpy((4 * x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)).cuda()
        b = torch.from_numpy((4 * y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)).cuda()
        for with_weights in (True, False):
            head = heads[with_weights]
            weights = (fw, fb, mw, mb) if with_weights else None
            calls = {"assign": lambda: head.assign(a, b), "match": lambda: head.match(a, b, min_score=-20.0),
                     "torch_assign": lambda: torch_assign(torch, a, b, weights, head.scale),
                     "torch_match": lambda: torch_match(torch, torch_assign(torch, a, b, weights, head.scale), -20.0)}
            times = interleaved(torch, calls, args.repeats, args.warmup)
            _, index, _ = head.match(a, b, min_score=-20.0)
            row = {"bench": "match_assignment", "rows": size, "dim": DIM, "with_weights": with_weights, "matches": int((index >= 0).sum().item()),
                   "max_abs_difference_to_torch": float((head.assign(a, b)[:size, :size] - torch_assign(torch, a, b, weights, head.scale)[:size, :size]).abs().max().item())}
            for label in calls:
                us_fields(row, label, times[label])
            yield row


def main():
    args = parser("--repeats", 30, 5, os.path.join(ROOT, "profiles", "match_assignment_bench.jsonl")).parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=True, extra={"device": torch.cuda.get_device_name(0)})


if __name__ == "__main__":
    main()
