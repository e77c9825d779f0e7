#!/usr/bin/env python3
"""upsample_flow (RAFT's convex flow upsampling, model.py:48-64) timing on the GPU box: one JSON line per shape.

    python scripts/bench_flow_upsample.py [--calls 100] [--warmup 10] [--cpu] [--out profiles/flow_upsample_bench.jsonl]

Shapes: B 1 at 60 x 94 (1/8 of the reference's example pair) and at RAFT's usual 55 x 128; B 12 at 60 x 94, the flows and masks of one
forward pass's 12 iterations stacked into one call.  Random flow and logits.
Fields (all times: one device-event pair per call, median over --calls after --warmup, as scripts/bench_raft_corr.py):
  kernel_ms / torch_ms                 (a) upsample_flow(flow, mask) and (b) the torch composition of model.py:48-64 on the same
                                       device and the same tensors.
  kernel_scaled_ms / torch_scaled_ms   (c) upsample_flow(flow, mask, 0.25) and (d) UpsampleFlow(flow, 0.25 * mask), the pass of
                                       update_block.py:66 included.
  *_rotating_ms                        the same calls over enough distinct input sets (--footprint-mb in all, default 640) that no
                                       call finds its mask in the 256 MB Infinity Cache; the plain figures reuse ONE set, which
                                       fits in it at B 1.
  kernel_gbps, kernel_rotating_gbps    the compulsory bytes 4 B H W (576 + 2 + 128) / time; copy_gbps is the measured float4 copy
                                       bandwidth of the MI355X guide (MI355X_MICROARCH.md: 6.29 TB/s, 79 % of the 8 TB/s HBM3E peak).
                                       A figure above it means the inputs came from cache, not from HBM.
  cpu_ms                               with --cpu: ONE call of the single-thread C restatement (tests/flow_upsample_ref.c) — labelled as
                                       such, not the reference's time.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import feature_tracker_amd as F  # noqa: E402
from feature_tracker_amd import _native  # noqa: E402
from scripts.benchlib import event_times, ms_fields, parser, write_rows  # noqa: E402
from tests import flow_upsample_ref as R  # noqa: E402
from tests.test_flow_upsample_cpu import torch_upsample  # noqa: E402

COPY_GBPS = 6290.0  # MI355X_MICROARCH.md: HBM3E, 6.29 TB/s measured with a float4 copy
SHAPES = [("eighth_example", 1, 60, 94), ("raft_55x128", 1, 55, 128), ("eighth_example_12_iterations", 12, 60, 94)]


def rows(args, torch):
    dev = torch.device("cuda")
    build = _native.build_info().get("source_hash", "?")
    for name, B, H, W in SHAPES:
        compulsory = 4 * B * H * W * (576 + 2 + 128)
        n_sets = max(2, -(-args.footprint_mb * 2 ** 20 // compulsory))
        g = torch.Generator().manual_seed(B * H + W)
        host = (torch.randn(B, 2, H, W, generator=g) * 3, torch.randn(B, 576, H, W, generator=g))
        sets = [(host[0].to(dev), host[1].to(dev))]
        for _ in range(n_sets - 1):
            sets.append((torch.randn(B, 2, H, W, device=dev) * 3, torch.randn(B, 576, H, W, device=dev)))
        flow, mask = sets[0]
        with torch.no_grad():
            variants = {
                "kernel": lambda f, m: F.upsample_flow(f, m),
                "torch": lambda f, m: torch_upsample(f, m),
                "kernel_scaled": lambda f, m: F.upsample_flow(f, m, 0.25),
                "torch_scaled": lambda f, m: torch_upsample(f, 0.25 * m),
            }
            t = {}
            for key, fn in variants.items():
                t[key] = event_times(torch, [lambda fn=fn: fn(flow, mask)], args.calls, args.warmup)
                t[key + "_rotating"] = event_times(torch, [lambda fn=fn, f=f, m=m: fn(f, m) for f, m in sets], args.calls, args.warmup)
            out = F.upsample_flow(flow, mask, 0.25).cpu().numpy()
        identical = R.same(out, R.upsample(host[0].numpy(), host[1].numpy(), 0.25))
        row = {"shape": name, "B": B, "H": H, "W": W, "compulsory_bytes": compulsory, "input_sets": n_sets}
        for key in t:
            ms_fields(row, key, t[key], spread=key.startswith("kernel"))
            if key.startswith("kernel"):
                row[key + "_gbps"] = round(compulsory / (t[key][0] * 1e-3) / 1e9, 1)
        row["copy_gbps"] = COPY_GBPS
        for a, b in (("kernel", "torch"), ("kernel_scaled", "torch_scaled"), ("kernel_rotating", "torch_rotating"), ("kernel_scaled_rotating", "torch_scaled_rotating")):
            row[a + "_speedup_vs_torch"] = round(t[b][0] / t[a][0], 2)
        row["identical_to_restatement"] = bool(identical)
        row["build"] = build
        if args.cpu:
            t0 = time.perf_counter()
            R.upsample(host[0].numpy(), host[1].numpy(), 0.25)
            row["cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["cpu_note"] = "one call of the single-thread C restatement (tests/flow_upsample_ref.c, gcc -O3), not the reference's time"
        yield row
        del sets, flow, mask
        torch.cuda.empty_cache()


def main():
    ap = parser("--calls", 100, 10)
    ap.add_argument("--footprint-mb", type=int, default=640, help="total size of the rotating input sets")
    ap.add_argument("--cpu", action="store_true", help="also time one call of the single-thread C restatement")
    args = ap.parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=False)


if __name__ == "__main__":
    main()
