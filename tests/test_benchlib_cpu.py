"""scripts/benchlib.py and scripts/bench_scenes.py without a device: the two timing loops on a stub in place of torch (it counts
synchronisations and hands out events with scripted elapsed times), the row helpers, the writer, the import discipline of the bench scripts,
and the shared inputs against the arrays the scripts' own generators gave before they were moved (tests/golden/bench_scenes/)."""
import ast
import glob
import importlib
import json
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from scripts import bench_scenes, benchlib  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "bench_scenes")
SCRIPTS = sorted(p for p in glob.glob(os.path.join(ROOT, "scripts", "bench_*.py")) if os.path.basename(p) != "bench_scenes.py")  # the programs


class StubTorch:
    """``cuda.synchronize`` and ``cuda.Event`` only; every event pair reports the next of ``elapsed``; ``log`` keeps the order of things."""

    def __init__(self, elapsed=()):
        stub, self.log, self.elapsed = self, [], list(elapsed)

        class Event:
            def __init__(self, enable_timing=False):
                assert enable_timing

            def record(self):
                stub.log.append("record")

            def synchronize(self):
                stub.log.append("event_sync")

            def elapsed_time(self, other):
                assert other is not self
                return stub.elapsed.pop(0)

        self.cuda = types.SimpleNamespace(synchronize=lambda: self.log.append("sync"), Event=Event)


def test_wall_times_times_the_calls_after_the_warmup(monkeypatch):
    torch, clock = StubTorch(), [0.0]
    monkeypatch.setattr(benchlib.time, "perf_counter", lambda: clock[0])

    def fn():  # call k takes k + 1 seconds of the stubbed clock
        torch.log.append("fn")
        clock[0] += torch.log.count("fn")

    times = benchlib.wall_times(torch, fn, 3, 2)
    assert torch.log.count("fn") == 5
    assert times == [3.0, 4.0, 5.0]
    assert torch.log == ["fn", "fn", "sync"] + ["fn", "sync"] * 3  # every timed call starts on a synchronised device and ends in its own
    assert benchlib.wall_time(torch, fn) == 6.0


@pytest.mark.parametrize("n_fns,calls,warmup", [(1, 7, 2), (1, 5, 0), (3, 8, 1), (3, 7, 5)])
def test_event_times_rotates_and_warms_every_entry(n_fns, calls, warmup):
    scripted = [float(v) for v in np.random.default_rng(calls).uniform(0.1, 9.0, calls)]
    torch = StubTorch(scripted)
    fns = [lambda k=k: torch.log.append(k) for k in range(n_fns)]
    got = benchlib.event_times(torch, fns, calls, warmup)
    order = [e for e in torch.log if isinstance(e, int)]
    n_warm = max(warmup, n_fns)
    assert order == [q % n_fns for q in range(n_warm)] + [q % n_fns for q in range(calls)]
    assert set(order[:n_warm]) == set(range(n_fns))
    assert torch.log[n_warm] == "sync" and torch.log[n_warm + 1:n_warm + 5] == ["record", 0, "record", "event_sync"]
    assert got == (float(np.median(scripted)), float(np.percentile(scripted, 10)), float(np.percentile(scripted, 90)))
    assert torch.elapsed == []


@pytest.mark.parametrize("repeats,per_entry", [(30, 30), (10, 9)])
def test_interleaved_is_round_major_and_truncates(monkeypatch, repeats, per_entry):
    torch, clock = StubTorch(), [0.0]
    monkeypatch.setattr(benchlib.time, "perf_counter", lambda: clock[0])

    def call(name):
        def fn():
            torch.log.append(name)
            clock[0] += 1.0
        return fn

    times = benchlib.interleaved(torch, {"b": call("b"), "a": call("a")}, repeats, 2)
    per_round = repeats // 3 + 2
    assert [e for e in torch.log if e != "sync"] == (["b"] * per_round + ["a"] * per_round) * 3
    assert list(times) == ["b", "a"] and all(len(v) == per_entry for v in times.values())
    assert len(benchlib.interleaved(torch, {"a": call("a")}, 10, 0, rounds=2)["a"]) == 10


def test_row_helpers_name_and_round():
    row = {"first": 1}
    benchlib.us_fields(row, "solve", [2.04e-6, 1.06e-6, 3.0e-6])
    assert row == {"first": 1, "solve_us_median": 2.0, "solve_us_min": 1.1} and list(row) == ["first", "solve_us_median", "solve_us_min"]
    assert benchlib.us_median([1e-6, 2.26e-6]) == 1.6
    row = {}
    benchlib.ms_fields(row, "fused", (1.23456, 1.00004, 2.99996))
    assert row == {"fused_ms": 1.2346}
    benchlib.ms_fields(row, "torch", (1.23456, 1.00004, 2.99996), spread=True)
    assert list(row) == ["fused_ms", "torch_ms", "torch_ms_p10", "torch_ms_p90"] and row["torch_ms_p10"] == 1.0 and row["torch_ms_p90"] == 3.0
    benchlib.ms_fields(row, "raw", (1.23456, 1.00004, 2.99996), spread=True, digits=None)
    assert (row["raw_ms"], row["raw_ms_p10"], row["raw_ms_p90"]) == (1.23456, 1.00004, 2.99996)
    values = [3.0, 1.0, 2.0, 10.0]
    assert benchlib.percentiles(values) == (float(np.median(values)), float(np.percentile(values, 10)), float(np.percentile(values, 90)))


def test_write_rows_modes(tmp_path, capsys):
    out = str(tmp_path / "new_directory" / "rows.jsonl")
    rows = [{"a": 1}, {"a": 2, "b": [1.5]}]
    assert benchlib.write_rows(iter(rows), out, append=True, extra={"device": "x"}) == [{"a": 1, "device": "x"}, {"a": 2, "b": [1.5], "device": "x"}]
    printed = capsys.readouterr().out.splitlines()
    assert [json.loads(line) for line in printed] == [{"a": 1, "device": "x"}, {"a": 2, "b": [1.5], "device": "x"}]
    assert list(json.loads(printed[1])) == ["a", "b", "device"]  # extra goes last
    assert open(out).read().splitlines() == printed
    benchlib.write_rows(rows[:1], out, append=True)
    assert [json.loads(line) for line in open(out)] == [{"a": 1, "device": "x"}, {"a": 2, "b": [1.5], "device": "x"}, {"a": 1}]
    benchlib.write_rows(rows[1:], out, append=False, extra={"build": "h"})
    assert [json.loads(line) for line in open(out)] == [{"a": 2, "b": [1.5], "build": "h"}]
    late = str(tmp_path / "late.jsonl")

    def measuring(append):
        yield {"a": 1}
        assert (open(late).read() == '{"a": 1}\n') if append else not os.path.exists(late)  # appended as measured / written at the end
        yield {"a": 2}

    benchlib.write_rows(measuring(True), late, append=True)
    assert open(late).read() == '{"a": 1}\n{"a": 2}\n'
    os.remove(late)
    benchlib.write_rows(measuring(False), late, append=False)
    assert open(late).read() == '{"a": 1}\n{"a": 2}\n'
    before = sorted(os.listdir(tmp_path))
    capsys.readouterr()
    benchlib.write_rows(rows, None, append=True)
    assert len(capsys.readouterr().out.splitlines()) == 2 and sorted(os.listdir(tmp_path)) == before


def test_parser_keeps_each_scripts_flags():
    args = benchlib.parser("--repeats", 30, 5, "profiles/x.jsonl").parse_args([])
    assert (args.repeats, args.warmup, args.out) == (30, 5, "profiles/x.jsonl")
    args = benchlib.parser("--calls", 100, 10).parse_args(["--calls", "7", "--warmup", "0", "--out", "y"])
    assert (args.calls, args.warmup, args.out) == (7, 0, "y")


@pytest.mark.parametrize("path", SCRIPTS, ids=[os.path.basename(p)[:-3] for p in SCRIPTS])
def test_script_imports_and_keeps_to_the_library(path):
    """Every script is imported for real (none touches a device at import time, so none needs the ``ast`` route for this); by ``ast`` none
    imports another bench script and none defines a ``timed`` or ``time_gpu`` of its own, nested functions included.  bench_configs.py is
    exempt from the last: it is built on bench.py's loop, not on the library's, and its closure of that name (events on the launch stream
    around a call with a reset or reshuffle before it) is none of the copies the library replaced."""
    name = os.path.basename(path)[:-3]
    module = importlib.import_module("scripts." + name)
    assert callable(module.main)
    for node in ast.walk(ast.parse(open(path).read())):
        imported = []
        if isinstance(node, ast.Import):
            imported = [alias.name for alias in node.names]
        elif isinstance(node, ast.ImportFrom):
            imported = [node.module or ""] + [f"{node.module}.{alias.name}" for alias in node.names]  # ``from scripts import bench_x`` too
        for target in imported:
            module_name = target.split(".")[-1]
            assert not module_name.startswith("bench_") or module_name == "bench_scenes", f"{name} imports {target}"
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and name != "bench_configs":
            assert node.name not in ("timed", "time_gpu"), f"{name} defines {node.name}"


@pytest.fixture(scope="module")
def golden():
    arrays = {}
    for name in ("scenes", "sequence", "weights"):
        with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
            arrays.update({key: f[key] for key in f.files})
    with open(os.path.join(GOLDEN, "tables.json")) as f:
        return arrays, json.load(f)


def test_scene_tables_are_the_scripts_own(golden):
    _, tables = golden
    as_json = lambda value: json.loads(json.dumps(value))  # noqa: E731  (tuples as lists, as the fixture has them)
    assert as_json(bench_scenes.IMAGE) == tables["IMAGE"] == tables["PNP_IMAGE"]
    assert as_json(bench_scenes.K) == tables["PNP_K"]
    assert as_json(bench_scenes.VIDEO_SHAPES) == tables["KLT_VIDEO_SHAPES"] and list(bench_scenes.VIDEO_SHAPES) == list(tables["KLT_VIDEO_SHAPES"])
    assert as_json(bench_scenes.RAFT_SHAPES) == tables["RAFT_SHAPES"]
    assert as_json(bench_scenes.CORR_SHAPES) == tables["RAFT_CORR_SHAPES"]
    assert [bench_scenes.DIM, bench_scenes.HEADS, bench_scenes.LAYERS] == [tables["DIM"], tables["HEADS"], tables["LAYERS"]]
    assert as_json(bench_scenes.SIZES) == tables["SIZES"] and as_json(bench_scenes.WIDTHS) == tables["WIDTHS"]


def test_scenes_are_bit_identical_to_the_scripts_own(golden):
    """Captured from the generators while they still stood in bench_epipolar.py, bench_pnp.py and bench_klt_video.py, each at a small
    argument: scene(16), scene(16), sequence(64, 48, 3)."""
    arrays, _ = golden
    ref, cur = bench_scenes.two_view_scene(16)
    X, uv = bench_scenes.landmark_scene(16)
    frames = np.stack(bench_scenes.sequence(64, 48, 3))
    for name, got in (("two_view_ref", ref), ("two_view_cur", cur), ("landmarks", X), ("landmark_uv", uv), ("sequence", frames)):
        assert got.dtype == arrays[name].dtype and np.array_equal(got, arrays[name]), name


def test_seeded_weights_are_bit_identical_to_the_scripts_own(golden, monkeypatch):
    """``state_dict`` has no size argument (D 256, nine layers: 30 MB), so the fixture keeps, one after the other in one vector, the
    [:2, :16] corner (or [:16]) of every tensor of layer 0 and of the last projection, and whole the small tensors drawn after all nine
    layers (``state_dict_kept`` names them): those are only the same if the draws before them were, in number and order.  The names and
    shapes of all 203 tensors are pinned by a digest.  ``lightglue_inputs`` continues on the same generator, as the scripts do, at n = 4
    (descriptors cut to 16 columns); ``make_state`` runs at widths of 2.  Tensors stay on the host here: ``.cuda()`` is made a no-op."""
    import hashlib

    import torch

    arrays, tables = golden
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    rng = np.random.default_rng(1)
    sd = bench_scenes.state_dict(torch, rng)
    names = "\n".join(f"{key} {list(t.shape)}" for key, t in sd.items())
    assert len(sd) == tables["state_dict_tensors"] and hashlib.sha256(names.encode()).hexdigest() == tables["state_dict_names_sha256"]
    kept = tables["state_dict_kept"]
    assert len(kept) == 22 + 5 and kept[-1] == list(sd)[-1] == "log_assignment.8.matchability.bias"

    def corner(key):
        t = sd[key].numpy()
        if key.startswith("transformers.") or t.size > 512:
            t = t[:2, :16] if t.ndim == 2 else t[:16]
        return t.ravel()

    got = np.concatenate([corner(key) for key in kept])
    assert got.dtype == arrays["state_dict"].dtype and np.array_equal(got, arrays["state_dict"])
    a, b, kp0, kp1 = (t.numpy() for t in bench_scenes.lightglue_inputs(torch, rng, 4, (640.0, 480.0)))
    assert a.shape == b.shape == (4, bench_scenes.DIM)
    assert np.array_equal(np.concatenate([t.ravel() for t in (a[:, :16], b[:, :16], kp0, kp1)]), arrays["lightglue_inputs"])
    state = bench_scenes.make_state(torch, (2, 2, 2, 2, 2, 2), 1)
    assert len(state) == 24 and np.array_equal(np.concatenate([t.numpy().ravel() for t in state.values()]), arrays["make_state"])
