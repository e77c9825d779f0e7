#!/usr/bin/env python3
"""OnDemandCorrelation against CorrelationPyramid (RAFT) on the GPU box: one JSON line per shape and per model.

    python scripts/bench_raft_corr_ondemand.py [--calls 50] [--warmup 5] [--iterations 12] [--out profiles/raft_corr_ondemand_bench.jsonl]

Correlation rows (`row`: "correlation"), B = 1, random features, random coordinates, at the three shapes of scripts/bench_raft_corr.py and at
1080p's feature map (C 256, 135 x 240, 4 levels, r 4).  Timed as there: one device-event pair per call, median / p10 / p90 over --calls
after --warmup.
  prepare_ms, lookup_ms            OnDemandCorrelation's construction (transpose + pools) and one fused lookup
  workspace_bytes                  what it holds
  on_demand_total_ms               prepare_ms + iterations * lookup_ms
  build_ms, all_pairs_lookup_ms    CorrelationPyramid's, where the volume can be allocated and built; else all_pairs_error says why not
  volume_bytes                     what the volume takes (computed, whether or not it was allocated)
  all_pairs_total_ms               build_ms + iterations * all_pairs_lookup_ms
  level0_identical                 the level-0 channels of the two lookups are bit-identical (where both ran)
Model rows (`row`: "forward"): the whole Raft of scripts/bench_raft.py's two shapes, once per mode (`correlation`), `forward_ms`.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import feature_tracker_amd as F  # noqa: E402
from feature_tracker_amd import _native  # noqa: E402
from scripts.bench_scenes import CORR_SHAPES  # noqa: E402
from scripts.bench_scenes import RAFT_SHAPES as MODEL_SHAPES  # noqa: E402
from scripts.benchlib import event_times, ms_fields, parser, write_rows  # noqa: E402
from tests.test_raft_encoder_cpu import make_image, make_raft_state  # noqa: E402

SHAPES = CORR_SHAPES + [("features_of_1080p_c256", 256, 135, 240, 4, 4)]


def rows(args, torch):
    dev = torch.device("cuda")
    n = args.iterations
    for name, C, H, W, L, r in SHAPES:
        g = torch.Generator().manual_seed(C * H)
        f0, f1 = torch.randn(1, C, H, W, generator=g).to(dev), torch.randn(1, C, H, W, generator=g).to(dev)
        coords = (torch.rand(1, 2, H, W, generator=g) * torch.tensor([W, H], dtype=torch.float32).view(1, 2, 1, 1)).float().to(dev)
        K = (2 * r + 1) ** 2
        row = {"row": "correlation", "shape": name, "B": 1, "C": C, "H": H, "W": W, "levels": L, "radius": r, "iterations": n}
        with torch.no_grad():
            od = F.OnDemandCorrelation(f0, f1, L, r)
            p_ms = event_times(torch, [lambda: F.OnDemandCorrelation(f0, f1, L, r)], args.calls, args.warmup)
            l_ms = event_times(torch, [lambda: od.lookup(coords)], args.calls, args.warmup)
            ms_fields(row, "prepare", p_ms, spread=True)
            ms_fields(row, "lookup", l_ms, spread=True)
            row.update(workspace_bytes=od.workspace_bytes, on_demand_total_ms=round(p_ms[0] + n * l_ms[0], 4))
            mine = od.lookup(coords)[:, :K].clone()
            row["volume_bytes"] = 4 * _native.corr_pyramid_layout(1, H, W, L)[0]
            try:
                cp = F.CorrelationPyramid(f0, f1, L, r)
                b_ms = event_times(torch, [lambda: F.CorrelationPyramid(f0, f1, L, r)], args.calls, args.warmup)
                a_ms = event_times(torch, [lambda: cp.lookup(coords)], args.calls, args.warmup)
                ms_fields(row, "build", b_ms, spread=True)
                ms_fields(row, "all_pairs_lookup", a_ms, spread=True)
                row["all_pairs_total_ms"] = round(b_ms[0] + n * a_ms[0], 4)
                row["on_demand_over_all_pairs"] = round(row["on_demand_total_ms"] / row["all_pairs_total_ms"], 3)
                row["level0_identical"] = bool(torch.equal(mine.view(torch.int32), cp.lookup(coords)[:, :K].view(torch.int32)))
                del cp
            except (RuntimeError, _native.FtkError) as e:  # out of memory, or a grid the build does not have
                row["all_pairs_error"] = str(e).splitlines()[0][:200]
            del od
        torch.cuda.empty_cache()
        yield row
    if not args.no_models:
        for name, widths, B, H, W, iterations in MODEL_SHAPES:
            state = {k: v.to(dev) for k, v in make_raft_state(widths, 1).items()}
            ref_image, cur_image = make_image(B, 1, H, W, 1).to(dev), make_image(B, 1, H, W, 2).to(dev)
            last = {}
            for mode in ("all_pairs", "on_demand"):
                model = F.Raft.from_state_dict(state, widths[3], widths[4], max_iterations=iterations, correlation=mode)
                with torch.no_grad():
                    ms = event_times(torch, [lambda: model(ref_image, cur_image)[-1]], max(args.calls // 2, 5), args.warmup)
                    last[mode] = model(ref_image, cur_image)[-1]
                row = {"row": "forward", "shape": name, "correlation": mode, "B": B, "H": H, "W": W, "iterations": iterations, "widths": list(widths)}
                ms_fields(row, "forward", ms, spread=True)
                if mode == "on_demand":
                    row["max_abs_between_modes"] = float((last["on_demand"] - last["all_pairs"]).abs().max())
                yield row
            del state, last
            torch.cuda.empty_cache()


def main():
    ap = parser("--calls", 50, 5)
    ap.add_argument("--iterations", type=int, default=12)
    ap.add_argument("--no-models", action="store_true", help="skip the whole-Raft rows")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_raft_corr_ondemand.py needs a HIP device"
    extra = dict(build=_native.build_info().get("source_hash", "?"), device=torch.cuda.get_device_name(0), calls=args.calls)
    write_rows(rows(args, torch), args.out, append=False, extra=extra)


if __name__ == "__main__":
    main()
