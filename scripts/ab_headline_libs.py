#!/usr/bin/env python3
"""A / B of library builds on the headline (config 2) in ONE process on one GPU:
    python scripts/ab_headline_libs.py parent=/path/libftk_parent.so,cand=/path/libftk_cand.so [rounds] [out.json]
Each build is loaded through its own copy of the package (FTK_LIB_PATH is read when a copy first loads its library), checked against the
CPU oracle (positions as uint32, status, iteration counts), and then timed in pairs: the FIRST build's timing loop, then a candidate's,
for every candidate, `rounds` times.  A timing loop is bench.py's: >= 10 ms of untimed launches, 200 launches between two synchronisations.
Naming the first build's file a second time (a copy under another name) gives the null pair: its spread is the run's own noise."""
import importlib.util, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

PATHS = dict(item.split("=", 1) for item in sys.argv[1].split(","))
LIBS = list(PATHS)
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 8
STEPS = 200
OUT = sys.argv[3] if len(sys.argv) > 3 else None


def load_pkg(name):
    os.environ["FTK_LIB_PATH"] = os.path.abspath(PATHS[name])
    alias = f"fta_{name}"
    pkg_dir = os.path.join(ROOT, "feature_tracker_amd")
    spec = importlib.util.spec_from_file_location(alias, os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[alias] = mod
    spec.loader.exec_module(mod)
    importlib.import_module(alias + ".device")
    native = importlib.import_module(alias + "._native")
    native.lib()
    return mod


def main():
    from tests import oracle_lib
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    runs = {}
    with torch.cuda.stream(stream):
        for name in LIBS:
            F = load_pkg(name)
            D, synth = F.device, F.synth
            cfg = synth.CONFIGS["config2"]
            n, w, h, levels, half = cfg["n"], cfg["width"], cfg["height"], cfg["levels"], cfg["half"]
            ref_img, cur_img = synth.make_image_pair(w, h, (3.3, -2.1))
            rl, cl = synth.build_pyramid(ref_img, levels), synth.build_pyramid(cur_img, levels)
            uv = synth.make_features(n, w, h, seed=12345, half=half)
            ctx = D.context_on_stream(stream, 0)
            opt = F.OpticalFlowOptions()
            opt.kMethod, opt.kPatchRowHalfSize, opt.kPatchColHalfSize, opt.kMaxTrackPointsNumber = cfg["method"], half, half, n
            klt = D.DeviceKlt(cfg["model"], opt, D.upload_pyramid(rl, ctx, dev), D.upload_pyramid(cl, ctx, dev), ctx)
            d_ref = torch.from_numpy(uv).to(dev)
            d_in, d_st = d_ref.clone(), torch.zeros(n, dtype=torch.uint8, device=dev)
            outs = [(torch.empty_like(d_ref), torch.empty_like(d_st)) for _ in range(2)]
            d_it = torch.zeros(n, dtype=torch.int32, device=dev)
            klt.track(d_ref, d_in, d_st, outs[0][0], outs[0][1], d_it)
            stream.synchronize()
            if "cpu" not in runs:
                runs["cpu"] = oracle_lib.klt_track_pyramid(cfg["model"], rl, cl, uv, method=cfg["method"], half=half, max_points=n)
            ok, cuv, cst, cit = runs["cpu"]
            launches = [klt.bind(d_ref, d_in, d_st, o[0], o[1], None) for o in outs]
            for k in range(20):
                launches[k & 1]()
            stream.synchronize()
            same = bool(np.array_equal(outs[1][0].cpu().numpy().view(np.uint32), cuv.view(np.uint32)) and np.array_equal(outs[1][1].cpu().numpy(), cst)
                        and np.array_equal(d_it.cpu().numpy().astype(np.uint32), cit))
            info = F._native.lib().ftk_build_info()
            print(json.dumps({"lib": name, "bit_identical": same, "build": info.decode() if info else None}), flush=True)
            runs[name] = dict(launches=launches, keep=(klt, ctx, d_ref, d_in, d_st, outs, d_it, F), same=same)

        def timed(name):
            launches = runs[name]["launches"]
            t_warm, k = time.perf_counter(), 0
            while k < 6 or time.perf_counter() - t_warm < 10e-3:
                launches[k & 1]()
                k += 1
            stream.synchronize()
            t0 = time.perf_counter()
            for k in range(STEPS):
                launches[k & 1]()
            stream.synchronize()
            return (time.perf_counter() - t0) / STEPS * 1e6

        base = LIBS[0]
        rows = []
        for r in range(ROUNDS):
            for cand in LIBS[1:]:
                a = timed(base)
                b = timed(cand)
                rows.append({"round": r, "cand": cand, "parent_us": round(a, 3), "cand_us": round(b, 3), "ratio": round(b / a, 4)})
                print(json.dumps(rows[-1]), flush=True)
    summary = {}
    for cand in LIBS[1:]:
        rr = [x["ratio"] for x in rows if x["cand"] == cand]
        summary[cand] = {"median_ratio": float(np.median(rr)), "min": min(rr), "max": max(rr), "all_favour_candidate": all(x < 1.0 for x in rr),
                         "bit_identical": runs[cand]["same"]}
    pp = [x["parent_us"] for x in rows]
    summary["parent"] = {"median_us": float(np.median(pp)), "min_us": min(pp), "max_us": max(pp), "rel_spread": (max(pp) - min(pp)) / float(np.median(pp)),
                         "bit_identical": runs[base]["same"]}
    print(json.dumps(summary, indent=1))
    if OUT:
        with open(OUT, "w") as f:
            json.dump({"rows": rows, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
