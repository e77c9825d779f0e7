#!/usr/bin/env python3
"""CorrelationPyramid (RAFT) timing on the GPU box: one JSON line per shape.

    python scripts/bench_raft_corr.py [--calls 100] [--warmup 10] [--cpu] [--out FILE]

Shapes: 1/8 of the reference's example pair (60 x 94) with C 128, 3 levels, r 3 and with C 256, 4 levels, r 4; RAFT's usual
55 x 128 (1/8 of 1024 x 440) with C 256, 4 levels, r 4.  B = 1, random features, random coordinates.
Fields:
  build_ms / lookup_ms            this library (CorrelationPyramid's build, one fused lookup), one device-event pair per call,
                                  median over --calls after --warmup.
  torch_build_ms / torch_lookup_ms the reference's torch composition on the same device (matmul, / C ** 0.5, avg_pool2d; the grid,
                                  grid_sample per level, cat, permute, contiguous of model.py:87-88), timed the same way.
  cpu_build_ms / cpu_lookup_ms     the single-thread C restatement (tests/raft_corr_ref.c), one call (with --cpu).
  build_tflops                     2 B (HW)^2 C / build time; floor_us: that work at the 157.3 TF f32 matrix peak.
  lookup_gbps                      (volume slabs touched are gathers served mostly by the caches, so this counts the compulsory
                                   bytes: coordinates read + output written) / lookup time.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import feature_tracker_amd as F  # noqa: E402
from feature_tracker_amd import _native  # noqa: E402
from scripts.bench_scenes import CORR_SHAPES as SHAPES  # noqa: E402
from scripts.benchlib import event_times, ms_fields, parser, write_rows  # noqa: E402
from tests import raft_corr_ref as R  # noqa: E402
from tests.test_raft_corr_cpu import torch_lookup, torch_pyramid  # noqa: E402

F32_PEAK = 157.3e12


def rows(args, torch):
    dev = torch.device("cuda")
    build = _native.build_info().get("source_hash", "?")
    for name, C, H, W, L, r in SHAPES:
        g = torch.Generator().manual_seed(C * H)
        f0, f1 = torch.randn(1, C, H, W, generator=g), torch.randn(1, C, H, W, generator=g)
        coords = (torch.rand(1, 2, H, W, generator=g) * torch.tensor([W, H], dtype=torch.float32).view(1, 2, 1, 1)).float()
        a0, a1, ac = f0.to(dev), f1.to(dev), coords.to(dev)
        with torch.no_grad():
            cp = F.CorrelationPyramid(a0, a1, L, r)
            ref = torch_pyramid(a0, a1, L)
            b_ms = event_times(torch, [lambda: F.CorrelationPyramid(a0, a1, L, r)], args.calls, args.warmup)
            l_ms = event_times(torch, [lambda: cp.lookup(ac)], args.calls, args.warmup)
            tb_ms = event_times(torch, [lambda: torch_pyramid(a0, a1, L)], args.calls, args.warmup)
            tl_ms = event_times(torch, [lambda: torch_lookup(ref, ac, r)], args.calls, args.warmup)
            out = cp.lookup(ac)
        want = R.build(f0.numpy(), f1.numpy(), L)
        identical = all(R.same(cp.correlation_pyramid[l][:, 0].cpu().numpy(), want[l]) for l in range(L))
        identical = identical and R.same(out.cpu().numpy(), R.lookup(want, coords.numpy(), r))
        HW = H * W
        flop = 2.0 * HW * HW * C
        K = (2 * r + 1) ** 2
        lookup_bytes = 4 * (2 * HW + L * K * HW)
        elements, _, _ = _native.corr_pyramid_layout(1, H, W, L)
        row = {"shape": name, "B": 1, "C": C, "H": H, "W": W, "levels": L, "radius": r}
        ms_fields(row, "build", b_ms, spread=True)
        ms_fields(row, "lookup", l_ms, spread=True)
        ms_fields(row, "torch_build", tb_ms)
        ms_fields(row, "torch_lookup", tl_ms)
        row.update({"build_vs_torch": round(b_ms[0] / tb_ms[0], 3), "lookup_speedup_vs_torch": round(tl_ms[0] / l_ms[0], 2),
                    "build_tflops": round(flop / (b_ms[0] * 1e-3) / 1e12, 2), "floor_us": round(flop / F32_PEAK * 1e6, 1),
                    "volume_bytes": 4 * elements, "level0_bytes": 4 * HW * HW,
                    "lookup_gbps": round(lookup_bytes / (l_ms[0] * 1e-3) / 1e9, 1), "identical_to_restatement": bool(identical), "build": build})
        if args.cpu:
            t = time.perf_counter()
            R.build(f0.numpy(), f1.numpy(), L)
            row["cpu_build_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            t = time.perf_counter()
            R.lookup(want, coords.numpy(), r)
            row["cpu_lookup_ms"] = round((time.perf_counter() - t) * 1e3, 2)
            row["cpu_note"] = "single-thread C restatement (tests/raft_corr_ref.c, gcc -O3), not the reference's time"
        yield row
        del cp, ref, out
        torch.cuda.empty_cache()


def main():
    ap = parser("--calls", 100, 10)
    ap.add_argument("--cpu", action="store_true", help="also time the single-thread C restatement")
    args = ap.parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=False)


if __name__ == "__main__":
    main()
