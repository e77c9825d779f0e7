#!/usr/bin/env python3
"""NNFeatureMatcher post-processing (mutual-best matching of a score matrix) timing on the GPU box: one JSON line per shape.

    python scripts/bench_nn_match.py [--calls 200] [--warmup 20] [--out FILE]

Shapes: 300^2 (the reference's default size), 1024^2, 2048^2, 4096^2 contiguous, and the [:-1, :-1] view of a 2049 x 2049 matrix
(LightGlue's layout: row stride 2049, so 4-byte loads).  B = 1, random normal scores.
Fields:
  us                 this library (the device entry on preallocated outputs, as a caller in a loop would use it), back to back: one device-event pair around --calls calls, divided by the count (the matrix stays
                     in whatever cache holds it: 300^2 .. 1024^2 fit an XCD's 4 MiB L2, 2048^2 (16 MB) the aggregate L2 / Infinity
                     Cache, 4096^2 (64 MB) only the 256 MiB Infinity Cache).
  cold_us            one call per event pair after a 1 GiB buffer has been rewritten (the matrix comes from HBM), median.
  gbps / hbm_frac    4 n_ref n_cur bytes / time, back to back, and as a fraction of the 8 TB/s HBM peak; cold_gbps / cold_hbm_frac
                     the same for the cold call — the only one of the two that speaks about HBM.
  torch_us           the same step with stock torch ops on the same device, same run: max over dim 1 and 0, gather, arange, two
                     compares, where (same results: checked).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import feature_tracker_amd as F  # noqa: E402
from feature_tracker_amd import _native  # noqa: E402
from feature_tracker_amd import device as D  # noqa: E402
from feature_tracker_amd.raft import _context  # noqa: E402
from scripts.benchlib import parser, write_rows  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = [("300", 300, 300, 0), ("1024", 1024, 1024, 0), ("2048", 2048, 2048, 0), ("4096", 4096, 4096, 0), ("2048_view_of_2049", 2048, 2048, 1)]


def torch_step(torch, s, min_score):
    """Stock torch: ties in max() are not specified to go to the lowest index, so this is a timing comparison; on distinct scores
    the results agree (checked by the caller)."""
    row_max, row_best = s.max(dim=1)
    col_best = s.max(dim=0).indices
    mutual = col_best.gather(0, row_best) == torch.arange(s.size(0), device=s.device)
    ok = mutual & ~(row_max < min_score)
    return torch.where(ok, row_best, torch.full_like(row_best, -1))


def rows(args, torch):
    dev = torch.device("cuda")
    build = _native.build_info().get("source_hash", "?")
    m = F.NNFeatureMatcher()
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)  # 1 GiB: four times the Infinity Cache

    def back_to_back(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.calls

    def cold(fn):
        us = []
        for _ in range(args.cold_calls):
            flush.add_(1.0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        return float(np.median(us))

    for name, n_ref, n_cur, pad in SHAPES:
        g = torch.Generator().manual_seed(n_ref + pad)
        full = (torch.randn(n_ref + pad, n_cur + pad, generator=g) * 4).to(dev)
        s = full[:n_ref, :n_cur]
        with torch.no_grad():
            _, idx, _ = m.match_scores(s)
            same = bool((idx.long() == torch_step(torch, s, -3.0)).all())
            ctx = _context(torch.cuda.current_device())
            s3 = s.unsqueeze(0)
            o_idx = torch.empty((1, n_ref), dtype=torch.int32, device=dev)
            o_st = torch.empty((1, n_ref), dtype=torch.uint8, device=dev)
            ours = lambda: D.nn_match_scores_device(ctx, s3, -3.0, o_idx, o_st)  # noqa: E731
            us = back_to_back(ours)
            t_us = back_to_back(lambda: torch_step(torch, s, -3.0))
            c_us = cold(ours)
            tc_us = cold(lambda: torch_step(torch, s, -3.0))
        nbytes = 4.0 * n_ref * n_cur
        row = {"shape": name, "n_ref": n_ref, "n_cur": n_cur, "row_stride": n_cur + pad, "bytes": int(nbytes),
               "us": round(us, 2), "cold_us": round(c_us, 2), "torch_us": round(t_us, 2), "torch_cold_us": round(tc_us, 2),
               "speedup_vs_torch": round(t_us / us, 2), "cold_speedup_vs_torch": round(tc_us / c_us, 2),
               "gbps": round(nbytes / us / 1e3, 1), "hbm_frac": round(nbytes / (us * 1e-6) / HBM_PEAK, 3),
               "cold_gbps": round(nbytes / c_us / 1e3, 1), "cold_hbm_frac": round(nbytes / (c_us * 1e-6) / HBM_PEAK, 3),
               "same_as_torch_on_distinct_scores": same, "build": build}
        yield row


def main():
    ap = parser("--calls", 200, 20)
    ap.add_argument("--cold-calls", type=int, default=10)
    args = ap.parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=False)


if __name__ == "__main__":
    main()
