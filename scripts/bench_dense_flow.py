#!/usr/bin/env python3
"""DenseOpticalFlow (Farneback) timing on the GPU box: one JSON line per workload.

    python scripts/bench_dense_flow.py [--calls 200] [--warmup 20] [--host-calls 30] [--cpu-calls 1] [--workload all] [--out FILE]

Workloads: "example" = the reference program's settings (tests/data/optical_flow pair, 752 x 480, 5 levels, half patch 2,
20 iterations); "vga4" = a 640 x 480 synthetic pair, 4 levels, the default options.
Fields:
  device_ms_median   ftk_dense_flow_device on resident pyramids and flow tensors, one device-event pair per call, median over
                     --calls calls after --warmup.
  host_call_ms       DenseOpticalFlow.Track with host images in and host flow out (device pyramid build from the host image,
                     the call, the download), wall clock, median over --host-calls.
  cpu_restatement_ms the single-thread C restatement (tests/dense_flow_ref.c, gcc -O3) on the same inputs — NOT the reference's
                     time (the reference library needs Eigen and un-vendored repos and is not built here).
  compulsory_bytes   the bytes every call must move at least once: both images of every level, the moment images written and
                     read once (32 B per pixel of both images), the flow planes written and read by the median (16 B per ref
                     pixel); the bilinear taps of the iterations are re-reads served by the caches and are not counted.
  hbm_fraction       compulsory_bytes / device time over the 8 TB/s HBM peak (MI355X_MICROARCH.md) — a floor, not a bound.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import feature_tracker_amd as F  # noqa: E402
from feature_tracker_amd import _native, synth  # noqa: E402
from feature_tracker_amd import device as D  # noqa: E402
from scripts.benchlib import parser, percentiles, write_rows  # noqa: E402
from tests import dense_flow_ref as R  # noqa: E402

HBM_PEAK = 8.0e12


def workloads():
    from PIL import Image
    data = os.path.join(ROOT, "tests", "data", "optical_flow")
    ref = np.array(Image.open(os.path.join(data, "ref_image.png")).convert("L"))
    cur = np.array(Image.open(os.path.join(data, "cur_image.png")).convert("L"))
    yield "example", ref, cur, 5, dict(kHalfPatchSize=2, kMaxIteration=20)
    ref, cur = synth.make_image_pair(640, 480, (3.3, -2.1))
    yield "vga4", ref, cur, 4, {}


def compulsory_bytes(rl, cl):
    b = 0
    for r, c in zip(rl, cl):
        b += r.size + c.size            # images
        b += 2 * 32 * (r.size + c.size)  # moments written, read once
        b += 2 * 16 * r.size             # raw flow written + read, smoothed written + read
    return b


def rows(args, torch):
    for name, ref, cur, levels, opts in workloads():
        if args.workload not in ("all", name):
            continue
        rl, cl = synth.build_pyramid(ref, levels), synth.build_pyramid(cur, levels)
        d = F.DenseOpticalFlow()
        for k, v in opts.items():
            setattr(d.options(), k, v)
        o = d.options()
        ropt = R.options(o.kMaxIteration, o.kHalfPatchSize, o.kMaxConvergeStep, o.kMaxDeltaFlowStep)
        # device-resident
        stream = torch.cuda.Stream()
        ctx = D.context_on_stream(stream)
        rp, cp = D.upload_pyramid(rl, ctx, "cuda"), D.upload_pyramid(cl, ctx, "cuda")
        out_r = torch.empty(ref.shape, dtype=torch.float32, device="cuda")
        out_c = torch.empty_like(out_r)
        torch.cuda.synchronize()
        times = []
        with torch.cuda.stream(stream):
            for i in range(args.warmup + args.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                D.dense_flow_device(ctx, o, rp, cp, out_r, out_c)
                e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    times.append(e0.elapsed_time(e1))
        dev_r, dev_c = out_r.cpu().numpy(), out_c.cpu().numpy()
        ctx.close()
        # host images in, host flow out
        host = []
        for i in range(args.host_calls + 3):
            t0 = time.perf_counter()
            ok, (fr, fc) = d.Track(F.ImagePyramid.build(ref, levels), F.ImagePyramid.build(cur, levels))
            t1 = time.perf_counter()
            if i >= 3:
                host.append((t1 - t0) * 1e3)
        # CPU restatement, single thread
        cpu = []
        for _ in range(max(args.cpu_calls, 1)):
            t0 = time.perf_counter()
            ok_c, fr_c, fc_c, _ = R.track_pyramid(rl, cl, ropt)
            cpu.append((time.perf_counter() - t0) * 1e3)
        identical = bool(ok and ok_c and R.same(fr, fr_c) and R.same(fc, fc_c) and R.same(dev_r, fr_c) and R.same(dev_c, fc_c))
        dev_ms, dev_p10, dev_p90 = percentiles(times)
        nbytes = compulsory_bytes(rl, cl)
        line = dict(workload=name, shape=[int(ref.shape[0]), int(ref.shape[1])], levels=levels, half_patch=o.kHalfPatchSize, max_iteration=o.kMaxIteration,
                    device_ms_median=round(dev_ms, 4), device_ms_p10=round(dev_p10, 4), device_ms_p90=round(dev_p90, 4),
                    device_calls=len(times), host_call_ms=round(float(np.median(host)), 4), cpu_restatement_ms=round(float(np.median(cpu)), 2),
                    cpu_restatement_note="single-thread C restatement (tests/dense_flow_ref.c, gcc -O3), not the reference's time",
                    speedup_vs_cpu_restatement=round(float(np.median(cpu)) / dev_ms, 1), compulsory_bytes=nbytes,
                    hbm_fraction=round(nbytes / (dev_ms * 1e-3) / HBM_PEAK, 5), identical_to_restatement=identical,
                    build=_native.build_info().get("source_hash"))
        yield line


def main():
    ap = parser("--calls", 200, 20)
    ap.add_argument("--host-calls", type=int, default=30)
    ap.add_argument("--cpu-calls", type=int, default=1)
    ap.add_argument("--workload", default="all", help="example | vga4 | all")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_dense_flow.py measures on a HIP device (no CPU fallback)"
    lines = write_rows(rows(args, torch), args.out, append=False)
    return 0 if all(l["identical_to_restatement"] for l in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
