"""The loud failures of the assignment head before any device is touched: the walk of tests/args_walk.py over
``device.match_assignment_device``; the refusals of ``MatchAssignment``; the agreement of header, library and binding; and the launch
plan through host/build/match_assignment_plan_cli."""
import types

import pytest

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

PLAN_CLI = A.plan_cli("match_assignment_plan_cli")


def _call(w, m=6, n=7, d=16, weights=True, counts=True, scale=0.5, row_stride=None):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    desc0, desc1 = w.t("desc0", "float32", m, d), w.t("desc1", "float32", n, d)
    wt = w.t("weights", "float32", d + 1, d) if weights else None
    bias = w.t("bias", "float32", d + 1) if weights else None
    c0 = w.t("count0", "int32", 1) if counts else None
    c1 = w.t("count1", "int32", 1) if counts else None
    clip = lambda v, hi: min(max(v, 1), hi)  # noqa: E731
    words = -(-N.match_assignment_workspace_bytes(clip(m, 4096), clip(n, 4096), clip(d, 1024), weights) // 8)
    stride = row_stride if isinstance(row_stride, int) and row_stride > n else n + 1
    return D.match_assignment_device(w.ctx, desc0, desc1, wt, bias, scale, c0, c1, w.t("workspace", "int64", words),
                                     w.t("scores", "float32", m * stride + n + 1), row_stride)


def test_entry_takes_no_pointer_of_an_unchecked_argument(monkeypatch):
    for kw in (dict(), dict(weights=False), dict(counts=False), dict(row_stride=12)):
        A.walk_call(monkeypatch, lambda w: _call(w, **kw), ["ftk_match_assignment_device"])


@pytest.mark.parametrize("kind", ["dtype", "shape", "device"])
def test_each_refused_tensor_stops_the_entry_before_the_library(monkeypatch, kind):
    def reshape(fake):  # (a row fewer is a valid call: a column fewer is not)
        return (fake.shape[0], fake.shape[1] - 1) if fake.name in ("desc0", "desc1") else A.one_row_fewer(fake)

    # (desc0 with a column fewer is a valid tensor: desc1, sized by it, is the one refused)
    A.refusal_sweep(monkeypatch, _call, kind, loose=("desc0", "desc1"), reshape=reshape)


def test_other_refusals(monkeypatch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    w = A.Walk(monkeypatch)
    for match, kw in (("FTK_MATCH_ASSIGNMENT_MAX_ROWS", dict(m=4097)), ("FTK_MATCH_ASSIGNMENT_MAX_ROWS", dict(n=4097)), ("FTK_MATCH_ASSIGNMENT_MAX_ROWS", dict(m=0)),
                      ("FTK_MATCH_ASSIGNMENT_MAX_DIM", dict(d=1025)), ("FTK_MATCH_ASSIGNMENT_MAX_DIM", dict(d=0, weights=False)),
                      ("scale must be a finite number > 0", dict(weights=False, scale=0.0)), ("scale must be", dict(weights=False, scale=float("nan"))),
                      ("scale must be", dict(weights=False, scale=float("inf"))), ("scale must be", dict(weights=False, scale=-0.5)),
                      ("scale must be", dict(weights=False, scale="big")), ("row_stride must be at least N \\+ 1 = 8", dict(row_stride=7)),
                      ("row_stride must be an integer", dict(row_stride=8.0)), ("row_stride must be", dict(row_stride=(1 << 24) + 1))):
        with pytest.raises(ValueError, match=match):
            _call(w, **kw)
    with pytest.raises(ValueError, match="weights and bias go together"):
        D.match_assignment_device(w.ctx, None, None, w.t("weights", "float32", 17, 16), None, 1.0, None, None, None, None)
    assert w.lib.calls == [] and w.unchecked_reads == []
    for kw in (dict(), dict(weights=False), dict(counts=False), dict(m=1, n=1, d=1), dict(m=4096, n=4096, d=4), dict(d=1024), dict(row_stride=8),
               dict(row_stride=1 << 24, m=1), dict(scale=float("nan"))):  # (scale is ignored with weights)
        _call(w, **kw)
    assert len(w.lib.calls) == 9
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    for match, call in (("dim must be an integer in 1", lambda: F.MatchAssignment.without_weights(0)), ("dim must be", lambda: F.MatchAssignment.without_weights(1025)),
                        ("dim must be", lambda: F.MatchAssignment.without_weights(64.0)), ("scale must be", lambda: F.MatchAssignment.without_weights(64, scale=0)),
                        ("scale must be", lambda: F.MatchAssignment.without_weights(64, scale=float("inf"))),
                        ("context_on_stream", lambda: F.MatchAssignment.without_weights(64, ctx=types.SimpleNamespace(handle=None)))):
        with pytest.raises(ValueError, match=match):
            call()
    head = F.MatchAssignment.without_weights(256)
    assert head.scale == 256 ** -0.25 and not head.with_weights and head.dim == 256
    sd = {"log_assignment.8.final_proj.weight": torch.zeros(16, 16), "log_assignment.8.final_proj.bias": torch.zeros(16),
          "log_assignment.8.matchability.weight": torch.zeros(1, 16), "log_assignment.8.matchability.bias": torch.zeros(1)}
    learned = F.MatchAssignment.from_state_dict(sd)
    assert learned.dim == 16 and learned.with_weights
    packed, bias = next(iter(learned._packed.values()))
    assert tuple(packed.shape) == (17, 16) and tuple(bias.shape) == (17,) and packed.is_contiguous()
    assert F.MatchAssignment.from_state_dict({k.replace("log_assignment.8.", "head."): v for k, v in sd.items()}, prefix="head.").dim == 16
    for match, change in (("lacks", {"log_assignment.8.final_proj.bias": None}), ("must be a float32 tensor", {"log_assignment.8.final_proj.weight": torch.zeros(16, 16).double()}),
                          ("must be \\[D, D\\]", {"log_assignment.8.final_proj.weight": torch.zeros(16, 15)}), ("must be \\[16\\]", {"log_assignment.8.final_proj.bias": torch.zeros(15)}),
                          ("must be \\[1, 16\\]", {"log_assignment.8.matchability.weight": torch.zeros(16)}), ("must be \\[1\\]", {"log_assignment.8.matchability.bias": torch.zeros(2)})):
        bad = {k: v for k, v in {**sd, **change}.items() if v is not None}
        with pytest.raises(ValueError, match=match):
            F.MatchAssignment.from_state_dict(bad)
    a, b = torch.zeros(6, 16), torch.zeros(7, 16)
    one = torch.zeros(1, dtype=torch.int32)
    for match, args, kw in (("^desc0 must be .*wrong dtype", (a.double(), b), {}), ("^desc1 must be .*dimension 1 is 15", (a, torch.zeros(7, 15)), {}),
                            ("^desc0 must be .*dimension 1 is 15", (torch.zeros(6, 15), b), {}), ("^desc0 must be .*strided view", (torch.zeros(6, 32)[:, ::2], b), {}),
                            ("^count0 must be .*wrong dtype", (a, b), dict(count0=one.long())), ("^count1 must be .*dimension 0 is 2", (a, b), dict(count1=torch.zeros(2, dtype=torch.int32))),
                            ("FTK_MATCH_ASSIGNMENT_MAX_ROWS", (torch.zeros(4097, 16), b), {}), ("^out must be a float32 tensor of shape \\[7, 8\\]", (a, b), dict(out=torch.zeros(7, 7))),
                            ("^out must be", (a, b), dict(out=torch.zeros(7, 16)[:, ::2])), ("is not out's row stride", (a, b), dict(out=torch.zeros(7, 8), row_stride=12)),
                            ("row_stride must be at least", (a, b), dict(row_stride=7)), ("no CPU fallback", (a, b), {}),
                            ("no CPU fallback", (a, b), dict(count0=one, count1=one, out=torch.zeros(7, 8)))):
        with pytest.raises(ValueError, match=match):
            learned.assign(*args, **kw)
    with pytest.raises(ValueError, match="min_score must be a number"):
        learned.match(a, b, min_score=float("nan"))
    with pytest.raises(ValueError, match="no CPU fallback"):
        learned.match(a, b, min_score=-3.0)
    assert recorder.calls == []


def test_header_library_and_binding_agree():
    import ctypes as C
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    header = A.header_library_and_binding_agree(("FTK_MATCH_ASSIGNMENT_MAX_ROWS", "FTK_MATCH_ASSIGNMENT_MAX_DIM"),
                                                {"ftk_match_assignment_workspace_bytes", "ftk_match_assignment_device"})
    assert "nn_feature_matcher.cpp:130-131" in header
    assert "MatchAssignment" in F.__all__ and callable(D.match_assignment_device)
    lib, out = N.lib(), C.c_int64()
    for m, n in ((1, 1), (31, 33), (64, 65), (130, 130), (300, 2048), (4096, 4096)):
        for d in (1, 3, 64, 65, 256, 1024):
            for weights in (0, 1):
                assert lib.ftk_match_assignment_workspace_bytes(m, n, d, weights, C.byref(out)) == 0
                assert out.value == N.match_assignment_workspace_bytes(m, n, d, bool(weights)) and out.value % 16 == 0
    bytes_of = lib.ftk_match_assignment_workspace_bytes
    assert bytes_of(0, 1, 4, 0, C.byref(out)) == -1 and bytes_of(1, 4097, 4, 0, C.byref(out)) == -1 and bytes_of(1, 1, 0, 0, C.byref(out)) == -1
    assert bytes_of(1, 1, 1025, 1, C.byref(out)) == -1 and bytes_of(1, 1, 4, 0, None) == -1
    assert lib.ftk_match_assignment_device(None, None, None, 1, None, 1, 1, None, None, 1.0, None, None, None, None, 0) == -1  # null context


def test_nothing_in_the_package_imports_the_restatement():
    A.nothing_in_the_package_imports("match_assignment_ref")


def _plan(m, n, d, weights, stride, aligned):
    """The plan restated (csrc/match_assignment_plan.cpp)."""
    if not (1 <= m <= 4096 and 1 <= n <= 4096):
        return {"refused": "rows"}
    if not 1 <= d <= 1024:
        return {"refused": "dim"}
    if stride != 0 and not n + 1 <= stride <= 1 << 24:
        return {"refused": "stride"}
    up16 = lambda v: (v + 15) & ~15  # noqa: E731
    w = bool(weights)
    off_z = up16(4 * (m + n) * d) if w else 0
    off_lse_row = off_z + (up16(4 * (m + n)) if w else 0)
    off_lse_col = off_lse_row + up16(4 * m)
    off_ls0 = off_lse_col + up16(4 * n)
    off_ls1 = off_ls0 + (up16(8 * m) if w else 0)
    return {"refused": "none", "row_stride": stride or n + 1, "vec": int(d % 4 == 0 and bool(aligned)), "gemm_threads": 256,
            "project_grid_x": -(-(m + n) // 128) if w else 0, "project_grid_y": -(-(d + 1) // 128) if w else 0, "sim_grid_x": -(-m // 128),
            "sim_grid_y": -(-n // 128), "norm_threads": 64, "norm_row_blocks": m, "norm_col_blocks": -(-n // 16), "norm_lds": 64 * 17 * 4,
            "finish_threads": 256, "finish_grid_x": -(-(n + 1) // 256), "finish_grid_y": -(-(m + 1) // 8), "launches": 4 if w else 3, "off_md": 0,
            "off_z": off_z, "off_lse_row": off_lse_row, "off_lse_col": off_lse_col, "off_ls0": off_ls0, "off_ls1": off_ls1,
            "bytes": off_ls1 + (up16(8 * n) if w else 0)}


def test_plan_cli_equals_the_restated_plan():
    from feature_tracker_amd import _native as N
    cases = [(m, n, d, weights, stride, aligned) for m, n in ((1, 1), (31, 33), (64, 65), (128, 129), (130, 130), (300, 2048), (4096, 4096), (0, 5), (3, 4097), (-1, -1))
             for d in (1, 2, 3, 64, 65, 256, 1024, 0, 1025) for weights in (0, 1) for stride in (0, n + 1, n + 5, n, 1 << 24, (1 << 24) + 1) for aligned in (0, 1)]
    plans = A.run_plan_tool(PLAN_CLI, cases)
    seen = set()
    for case, got in zip(cases, plans):
        want = _plan(*case)
        assert got == {k: str(v) for k, v in want.items()}, (case, got, want)
        seen.add(want["refused"])
        if want["refused"] == "none":
            assert want["bytes"] == N.match_assignment_workspace_bytes(case[0], case[1], case[2], bool(case[3]))
            assert want["sim_grid_y"] <= 65535 and want["finish_grid_y"] <= 65535 and want["norm_lds"] <= 65536
    assert seen == {"none", "rows", "dim", "stride"}
