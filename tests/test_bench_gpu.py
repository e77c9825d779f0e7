"""bench.py itself on the GPU box, in the shapes the driver runs it — so that the driver's suite exercises what its bench run will meet.

* FTK_BENCH_FORCE_DIST=1 at world size 1 takes the N > 1 code path: process group on RCCL, one all-gather per step, the K steps captured
  in one HIP graph with the gather on a side stream, and the `config5_sharded` object (BASELINE configs[4]: features sharded over the
  ranks, torch.distributed AND the C ABI's own ncclAllGather) — VERDICT r4 item 3.
* the N = 1 --full line carries `roofline`, `cpu_baseline` and the `real_images` rows (the reference's example pair), every row
  bit-identical to the oracle — VERDICT r4 item 1.
* a plain run (no --full) prints only the headline fields, and --dump-outputs writes what its last timed step returned.
The bench process is a CHILD of the test process (one GPU process at a time beside pytest itself)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(argv, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env)
    res = subprocess.run([sys.executable, BENCH, *argv], env=e, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return lines[0]


def test_forced_dist_run_carries_config5_sharded_through_rccl():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    line = _run(["--steps", "5", "--warmup", "2", "--config5-total", "40000", "--full"], FTK_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    assert line["n_gpus"] == 1 and line["rccl_ranks"] == 1 and line["scaling"] == "weak"
    assert "all-gather" in line["config"]["parallelism"]
    assert line["parity"]["bit_identical"] and line["parity"]["last_launch_bit_identical"]
    c5 = line["config5_sharded"]
    assert "error" not in c5, c5
    assert c5["backend"] == "nccl" and c5["rccl_ranks"] == 1 and c5["total_features"] == 40000 and c5["features_per_rank"] == 40000
    t = c5["torch"]
    assert t["gathered_equals_unsharded_bitwise"] is True and t["ms_per_step"] > 0 and t["all_gather_us"] > 0 and t["kernel_us"] > 0
    nat = c5["native_comm"]
    assert "error" not in nat and "skipped" not in nat, nat
    assert nat["gathered_equals_unsharded_bitwise"] is True and nat["rccl_ranks"] == 1 and nat["ms_per_step"] > 0


def test_default_line_carries_roofline_cpu_baseline_and_real_image_rows():
    line = _run(["--steps", "20", "--warmup", "5", "--no-configs-leg", "--no-tree-leg", "--no-upload-leg", "--full"])
    assert line["n_gpus"] == 1 and line["parity"]["bit_identical"]
    assert line["roofline"]["bound"] == "hbm" and 0 < line["roofline"]["frac"] < 1
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["cores"] == 1
    real = line["real_images"]
    assert "skipped" not in real, real
    assert len(real["rows"]) == 18 and real["all_bit_identical"], {k: v["bit_identical"] for k, v in real["rows"].items()}
    for key, row in real["rows"].items():
        assert row["ms_per_step"] > 0 and row["host_call_ms"] > row["ms_per_step"] * 0.5, (key, row)
    assert "config5_sharded" not in line  # N = 1 without the forced process group: no collective anywhere


def test_plain_line_is_lean_and_dumps_the_last_step_bit_identical_to_the_oracle(tmp_path, oracle):
    import numpy as np

    from feature_tracker_amd import synth

    out = tmp_path / "outputs"
    line = _run(["--steps", "7", "--warmup", "2", "--dump-outputs", str(out)])
    assert line["n_gpus"] == 1 and line["steps"] == 7 and line["warmup"] == 2
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["unit"] == "tracked features/s"
    assert line["ms_per_step"] > 0 and abs(line["value"] - 2000 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    moved = {"roofline", "roofline_valu", "parity", "cpu_baseline", "throughput_mode", "with_pyramid_upload", "configs", "host_call", "real_images",
             "config5_sharded"}
    assert not moved & set(line), sorted(moved & set(line))
    uv, st = np.load(out / "cur_uv.npy"), np.load(out / "status.npy")
    assert uv.dtype == np.float32 and uv.shape == (2000, 2) and st.dtype == np.float32 and st.shape == (2000,)
    # the same seeded inputs through the oracle: the dumped result is the oracle's, bit for bit
    cfg = synth.CONFIGS["config2"]
    ref_img, cur_img = synth.make_image_pair(cfg["width"], cfg["height"], (3.3, -2.1))
    ref_levels, cur_levels = synth.build_pyramid(ref_img, cfg["levels"]), synth.build_pyramid(cur_img, cfg["levels"])
    uv0 = synth.make_features(cfg["n"], cfg["width"], cfg["height"], seed=12345, half=cfg["half"])
    ok, c, s, _ = oracle.klt_track_pyramid(cfg["model"], ref_levels, cur_levels, uv0, method=cfg["method"], half=cfg["half"], max_points=cfg["n"])
    assert np.array_equal(uv.view(np.uint32), c.view(np.uint32)) and np.array_equal(st, s.astype(np.float32))
