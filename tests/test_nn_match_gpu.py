"""NNFeatureMatcher's post-processing on the device against the scalar restatement (tests/nn_match_ref.c): EXACT
equality of match_index, status and the bytes of matched_uv — comparisons only, so no tolerance and nothing left out.  Through the
C ABI's host entries (numpy), the torch entries (device tensors, torch's current stream) and the C++ class (nn_match_cli)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import nn_match_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "feature_tracker_amd", "host", "build", "nn_match_cli")
DEV = "cuda"


def uv_for(n_cur, seed=3):
    rng = np.random.default_rng(seed)
    uv = rng.random((n_cur, 2), dtype=np.float32) * np.float32(640)
    if n_cur > 2:
        uv[1, 0], uv[2, 1] = np.float32("nan"), np.float32(-0.0)  # carried bit for bit
    return uv


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_scores(m, scores_np, min_score, scores_t=None, what=""):
    """One item or a batch through the torch entry (and the pixel fill), against the restatement."""
    m.options().kMinValidMatchScore = min_score
    t = torch.from_numpy(np.ascontiguousarray(scores_np)).to(DEV) if scores_t is None else scores_t
    batched = scores_np.ndim == 3
    n_cur = scores_np.shape[-1]
    B = scores_np.shape[0] if batched else 1
    uv = np.stack([uv_for(n_cur, 10 + b) for b in range(B)]) if batched else uv_for(n_cur)
    ok, idx, st, muv = m.match_scores(t, uv_cur=torch.from_numpy(uv).to(DEV))
    want_idx, want_st = R.match_scores(scores_np, min_score)
    assert ok
    assert np.array_equal(idx.cpu().numpy(), want_idx), what
    assert np.array_equal(st.cpu().numpy(), want_st), what
    got = muv.cpu().numpy()
    if batched:
        for b in range(B):
            assert same_bytes(got[b], R.fill(want_idx[b], uv[b])), what
    else:
        assert same_bytes(got, R.fill(want_idx, uv)), what


# ---- the hand-derived cases through all three entries ----

@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_hand_cases_torch_and_host_entries(ftk, case):
    _, scores, min_score, expected = case
    m = ftk.NNFeatureMatcher()
    check_scores(m, scores, min_score)
    m.options().kMinValidMatchScore = min_score
    uv = uv_for(scores.shape[1])
    ok, idx, st, muv = m.match_scores(scores, uv_cur=uv)  # numpy: ftk_nn_match_scores
    assert ok and idx.tolist() == expected
    assert st.tolist() == [R.TRACKED if j >= 0 else R.LARGE_RESIDUAL for j in expected]
    assert same_bytes(muv, R.fill(idx, uv))


def cli_uv(n_cur):
    return np.float32([[j + 0.25, 1000.0 - j] for j in range(n_cur)]).reshape(n_cur, 2)


def run_cli(args, n_ref, n_cur):
    r = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=dict(os.environ, FTK_NO_WARMUP="1"))
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and lines[0] == "ok 1", r.stdout + r.stderr
    st = [int(x) for x in lines[1:1 + n_ref]]
    muv = np.array([[int(w, 16) for w in l.split()] for l in lines[1 + n_ref:1 + n_ref + n_cur]], dtype=np.uint32).reshape(n_cur, 2)
    return st, muv


@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_hand_cases_cpp_class(ftk, case, tmp_path):
    _, scores, min_score, expected = case
    assert os.path.exists(CLI), "host layer not built"
    n_ref, n_cur = scores.shape
    padded = np.full((n_ref + 1, n_cur + 1), 99.0, np.float32)  # LightGlue's layout: the dustbins would win every row if they were read
    padded[:n_ref, :n_cur] = scores
    path = tmp_path / "scores.f32"
    padded.reshape(-1)[:(n_ref - 1) * (n_cur + 1) + n_cur].tofile(path)
    bits = "%08x" % int(np.float32(min_score).view(np.uint32))
    st, muv = run_cli(["scores", n_ref, n_cur, n_cur + 1, bits, path], n_ref, n_cur)
    assert st == [R.TRACKED if j >= 0 else R.LARGE_RESIDUAL for j in expected]
    assert np.array_equal(muv, R.fill(np.int32(expected), cli_uv(n_cur)).view(np.uint32))


@pytest.mark.parametrize("case", R.list_cases(), ids=lambda c: c[0])
def test_list_cases_all_entries(ftk, case, tmp_path):
    _, matches, n_ref, n_cur, expected = case
    matches = np.asarray(matches, dtype=np.int64).reshape(-1, 2)
    want_st = [R.TRACKED if j >= 0 else R.LARGE_RESIDUAL for j in expected]
    m = ftk.NNFeatureMatcher()
    uv = uv_for(n_cur)
    ok, idx, st, muv = m.match_list(torch.from_numpy(matches).to(DEV), n_ref, n_cur, uv_cur=torch.from_numpy(uv).to(DEV))
    assert ok and idx.cpu().tolist() == expected and st.cpu().tolist() == want_st
    assert same_bytes(muv.cpu().numpy(), R.fill(np.int32(expected), uv))
    ok, idx, st, muv = m.match_list(matches, n_ref, n_cur, uv_cur=uv)  # numpy: ftk_nn_match_list
    assert ok and idx.tolist() == expected and st.tolist() == want_st and same_bytes(muv, R.fill(np.int32(expected), uv))
    path = tmp_path / "matches.i64"
    matches.tofile(path)
    cst, cmuv = run_cli(["list", n_ref, n_cur, matches.shape[0], path], n_ref, n_cur)
    assert cst == want_st and np.array_equal(cmuv, R.fill(np.int32(expected), cli_uv(n_cur)).view(np.uint32))


# ---- sizes, strides, alignment ----

SIZES = [(1, 1), (1, 300), (300, 1), (15, 17), (16, 256), (17, 257), (63, 255), (64, 1023), (65, 1025), (127, 513), (129, 40), (300, 300), (301, 299),
         (1000, 37), (37, 1000), (1024, 1024), (1025, 2049), (2049, 1025), (4096, 4096), (4095, 4097), (4096, 3)]


@pytest.mark.parametrize("n_ref,n_cur", SIZES, ids=lambda v: str(v))
def test_sizes_contiguous_strided_misaligned(ftk, n_ref, n_cur):
    m = ftk.NNFeatureMatcher()
    rng = np.random.default_rng(n_ref * 10007 + n_cur)
    batches = (1, 3) if n_ref * n_cur <= 1100 * 1100 else (1,)
    for B in batches:
        # heavy quantisation (ties everywhere), with and without NaN / inf / +-0, and distinct random scores
        for kind in ("quantised", "specials", "random"):
            if kind == "random":
                full = rng.standard_normal((B, n_ref + 1, n_cur + 1)).astype(np.float32) * np.float32(4)
            else:
                full = R.quantised(rng, (B, n_ref + 1, n_cur + 1), 8, 0.01 if kind == "specials" else 0.0, kind == "specials")
            full[:, -1, :] = np.float32("inf")  # dustbins: must never be read into a result
            full[:, :, -1] = np.float32("inf")
            view = full[:, :-1, :-1]
            thr = float(rng.choice([-3.0, 0.0, -100.0]))
            what = f"{n_ref} x {n_cur}, B {B}, {kind}"
            full_t = torch.from_numpy(full).to(DEV)
            check_scores(m, view, thr, scores_t=full_t[:, :-1, :-1], what=what + ", strided view")
            if kind == "quantised":
                check_scores(m, view, thr, what=what + ", contiguous")
                flat = torch.empty(view.size + 1, dtype=torch.float32, device=DEV)
                off = flat[1:].view(B, n_ref, n_cur)
                off.copy_(torch.from_numpy(np.ascontiguousarray(view)))
                assert off.data_ptr() % 16 == 4
                check_scores(m, view, thr, scores_t=off, what=what + ", misaligned base")
                if B == 1:
                    check_scores(m, view[0], thr, what=what + ", 2-D")


def test_one_repeated_value(ftk):
    """Every key of every row and column ties: the lowest index must win through every merge (lanes, waves, tiles, atomics)."""
    m = ftk.NNFeatureMatcher()
    for n_ref, n_cur, value in ((2500, 3000, 0.5), (700, 4000, -0.0), (3000, 129, float("-inf")), (513, 513, float("nan"))):
        s = np.full((n_ref, n_cur), value, np.float32)
        thr = float("-inf") if value != value or value == float("-inf") else -3.0
        check_scores(m, s, thr, what=f"all {value}")
        m.options().kMinValidMatchScore = thr
        ok, idx, st = m.match_scores(torch.from_numpy(s).to(DEV))
        assert idx.cpu().tolist() == [0] + [-1] * (n_ref - 1)  # row 0 takes column 0; every other row also wants column 0


def test_workspace_is_left_clean(ftk):
    """Two different problems back to back on one context, the second smaller than the first and with lower scores everywhere:
    any key left behind by the first would win in the second."""
    m = ftk.NNFeatureMatcher()
    rng = np.random.default_rng(77)
    big = (rng.standard_normal((3, 900, 1100)).astype(np.float32) + np.float32(50))
    small = (rng.standard_normal((2, 300, 260)).astype(np.float32) - np.float32(50))
    check_scores(m, big, -3.0, what="first")
    check_scores(m, small, -1000.0, what="second, smaller")
    matches = rng.integers(0, 250, size=(5000, 2)).astype(np.int64)
    ok, idx, st = m.match_list(torch.from_numpy(matches).to(DEV), 250, 250)
    want = R.match_list(matches, 250, 250)
    assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(st.cpu().numpy(), want[1])
    check_scores(m, small[0], -1000.0, what="after list mode")
    few = np.int64([[3, 4]])
    ok, idx, st = m.match_list(torch.from_numpy(few).to(DEV), 250, 250)
    assert np.array_equal(idx.cpu().numpy(), R.match_list(few, 250, 250)[0])


def test_list_mode_many_duplicates(ftk):
    """100 000 rows onto 1 000 references: the largest k must win whatever order the device applies them in."""
    rng = np.random.default_rng(4)
    matches = rng.integers(-50, 1100, size=(100000, 2)).astype(np.int64)
    matches[::97, 0] += 1 << 33
    m = ftk.NNFeatureMatcher()
    uv = uv_for(1000)
    ok, idx, st, muv = m.match_list(torch.from_numpy(matches).to(DEV), 1200, 1000, uv_cur=torch.from_numpy(uv).to(DEV))
    want_idx, want_st = R.match_list(matches, 1200, 1000)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(st.cpu().numpy(), want_st)
    assert same_bytes(muv.cpu().numpy(), R.fill(want_idx, uv))


def test_pixel_write_beyond_n_cur_is_skipped(ftk):
    """n_ref > n_cur in score mode: a matched row i >= n_cur keeps its match_index and status, and matched_uv (n_cur entries) is not
    written for it — the reference's unchecked write there is undefined."""
    s = np.full((6, 2), -9.0, np.float32)
    s[5, 1] = 4.0  # row 5 <-> column 1, mutual
    s[0, 0] = 3.0
    m = ftk.NNFeatureMatcher()
    uv = np.float32([[1, 2], [3, 4]])
    ok, idx, st, muv = m.match_scores(torch.from_numpy(s).to(DEV), uv_cur=torch.from_numpy(uv).to(DEV))
    assert idx.cpu().tolist() == [0, -1, -1, -1, -1, 1] and st.cpu().tolist() == [1, 2, 2, 2, 2, 1]
    assert muv.shape == (2, 2) and muv.cpu().tolist() == [[1, 2], [3, 4]]


def test_graph_capture_and_replays(ftk):
    """Captured once, replayed twice with the scores and pixels changed in place: no allocation and no synchronisation inside."""
    m = ftk.NNFeatureMatcher()
    rng = np.random.default_rng(31)
    B, n_ref, n_cur = 2, 333, 290
    full = torch.empty((B, n_ref + 1, n_cur + 1), dtype=torch.float32, device=DEV)
    uv = torch.empty((B, n_cur, 2), dtype=torch.float32, device=DEV)
    matches = torch.empty((400, 2), dtype=torch.int64, device=DEV)

    def fresh():
        f = R.quantised(rng, (B, n_ref + 1, n_cur + 1), 6)
        u = rng.random((B, n_cur, 2), dtype=np.float32)
        k = rng.integers(-5, 300, size=(400, 2)).astype(np.int64)
        full.copy_(torch.from_numpy(f))
        uv.copy_(torch.from_numpy(u))
        matches.copy_(torch.from_numpy(k))
        return f, u, k

    def run():
        a = m.match_scores(full[:, :-1, :-1], uv_cur=uv)
        b = m.match_list(matches, n_ref, n_cur, uv_cur=uv[0])
        return a[1:], b[1:]

    fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()  # sizes the key workspace outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        (idx, st, muv), (lidx, lst, lmuv) = run()
    for _ in range(2):
        f, u, k = fresh()
        g.replay()
        torch.cuda.synchronize()
        want_idx, want_st = R.match_scores(f[:, :-1, :-1], -3.0)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(st.cpu().numpy(), want_st)
        for b in range(B):
            assert same_bytes(muv[b].cpu().numpy(), R.fill(want_idx[b], u[b]))
        wl = R.match_list(k, n_ref, n_cur)
        assert np.array_equal(lidx.cpu().numpy(), wl[0]) and np.array_equal(lst.cpu().numpy(), wl[1])
        assert same_bytes(lmuv.cpu().numpy(), R.fill(wl[0], u[0]))


def test_capture_refuses_to_grow_the_workspace(ftk):
    """A capture that meets a key workspace that is too small gets an error naming the fix, not an allocation inside the graph."""
    from feature_tracker_amd import _native
    ctx = ftk.Context()  # a fresh context: no workspace yet
    m = ftk.NNFeatureMatcher(ctx)
    s = torch.zeros((40, 50), dtype=torch.float32, device=DEV)
    idx = torch.empty((1, 40), dtype=torch.int32, device=DEV)
    st = torch.empty((1, 40), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = _native.lib().ftk_nn_match_scores_device(ctx.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(s.data_ptr()), 1, 40, 50, 50, 0,
                                                      -3.0, C.c_void_p(idx.data_ptr()), C.c_void_p(st.data_ptr()))
        message = _native.lib().ftk_last_error(ctx.handle).decode()
        s.add_(1.0)  # the capture itself stays valid
    assert rc == -4 and "before the capture" in message and "captured" in message
    ok, idx2, st2 = m.match_scores(s)  # outside a capture the same call allocates and runs
    assert ok and idx2.cpu().tolist() == [0] + [-1] * 39


def test_size_validation_before_any_launch(ftk):
    from feature_tracker_amd import _native
    lib = _native.lib()
    ctx = ftk.default_context()
    s = torch.zeros(64, dtype=torch.float32, device=DEV)
    idx = torch.full((8,), 5, dtype=torch.int32, device=DEV)
    st = torch.full((8,), 9, dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def scores(batch, n_ref, n_cur, row_stride, batch_stride, d=p(s)):
        return lib.ftk_nn_match_scores_device(ctx.handle, stream, d, batch, n_ref, n_cur, row_stride, batch_stride, -3.0, p(idx), p(st))

    assert scores(1, 4, 0, 4, 0) == -1 and "n_cur 0" in lib.ftk_last_error(ctx.handle).decode()  # the reference would read an empty row
    assert scores(1, -1, 4, 4, 0) == -1
    assert scores(1, 4, 4, 3, 0) == -1 and "row stride" in lib.ftk_last_error(ctx.handle).decode()   # rows would overlap
    assert scores(2, 4, 4, 4, 15) == -1 and "batch stride" in lib.ftk_last_error(ctx.handle).decode()
    assert scores(65536, 1, 1, 1, 1) == -1
    assert scores(1, 4, 4, 4, 0, None) == -1
    assert scores(1, 0, 4, 4, 0) == 0 and scores(0, 4, 4, 4, 0) == 0  # nothing to do: no launch, nothing written
    assert lib.ftk_nn_match_list_device(ctx.handle, stream, None, 3, 4, 4, p(idx), p(st)) == -1
    assert lib.ftk_nn_match_list_device(ctx.handle, stream, p(s), -1, 4, 4, p(idx), p(st)) == -1
    assert lib.ftk_nn_fill_pixels_device(ctx.handle, stream, p(idx), 4, p(s), 4, p(s)) == -1 and "alias" in lib.ftk_last_error(ctx.handle).decode()
    assert lib.ftk_nn_fill_pixels_device(ctx.handle, stream, p(idx), 4, p(s), -4, p(st)) == -1
    torch.cuda.synchronize()
    assert idx.cpu().tolist() == [5] * 8 and st.cpu().tolist() == [9] * 8  # no refused call wrote anything
    m = ftk.NNFeatureMatcher()
    with pytest.raises(_native.FtkError):
        m.match_scores(torch.zeros((3, 0), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        m.match_scores(torch.zeros((3, 4), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        m.match_scores(torch.zeros((4, 3), dtype=torch.float32, device=DEV).t())  # column stride 4
    assert m.match_scores(torch.zeros((0, 4), dtype=torch.float32, device=DEV))[0] is False  # nn_feature_matcher.cpp:92
    ok = C.c_int(7)
    assert lib.ftk_nn_match_scores(ctx.handle, None, 1, 0, 3, 3, 0, -3.0, None, None, C.byref(ok)) == 0 and ok.value == 0
