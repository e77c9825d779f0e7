"""NNFeatureMatcher's post-processing without a device: the scalar restatement the kernels are held to
(tests/nn_match_ref.c) against hand-derived answers and an independent pure-Python double loop; the launch plan nn_match_plan over a
grid of shapes; the ABI surface."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import nn_match_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_EXE = os.path.join(ROOT, "feature_tracker_amd", "host", "build", "match_plan_cli")
NN_SYMBOLS = ("ftk_nn_match_scores_device", "ftk_nn_match_list_device", "ftk_nn_fill_pixels_device", "ftk_nn_match_scores", "ftk_nn_match_list")


# ---- the restatement ----

@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_restatement_hand_cases(case):
    _, scores, min_score, expected = case
    idx, st = R.match_scores(scores, min_score)
    assert idx.tolist() == expected
    assert st.tolist() == [R.TRACKED if j >= 0 else R.LARGE_RESIDUAL for j in expected]
    py_idx, py_st = R.match_scores_python(scores, min_score)
    assert py_idx.tolist() == expected and py_st.tolist() == st.tolist()


def test_restatement_strided_view_equals_its_copy():
    rng = np.random.default_rng(5)
    full = R.quantised(rng, (3, 18, 14))
    view = full[:, :-1, :-1]
    a = R.match_scores(view, -3.0)
    b = R.match_scores(np.ascontiguousarray(view), -3.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def quantised_cases():
    rng = np.random.default_rng(20240611)
    cases = []
    for n_ref, n_cur in itertools.product((1, 2, 3, 7, 16, 33), (1, 2, 5, 8, 31)):
        for levels, specials, nan_rate in ((2, False, 0.0), (8, False, 0.0), (8, True, 0.0), (3, False, 0.2)):
            cases.append((R.quantised(rng, (n_ref, n_cur), levels, nan_rate, specials), float(rng.choice([-3.0, 0.0, -1e30, np.nan, -np.inf]))))
    return cases


def test_restatement_against_python_loop_on_quantised_scores():
    ties = 0
    for scores, thr in quantised_cases():
        idx, st = R.match_scores(scores, thr)
        py_idx, py_st = R.match_scores_python(scores, thr)
        assert np.array_equal(idx, py_idx) and np.array_equal(st, py_st), (scores, thr)
        ties += int(scores.size > len(np.unique(scores[~np.isnan(scores)])))
    assert ties > 80  # the cases do tie


def test_quantised_scores_catch_the_ge_mutant():
    """`>=` instead of `>` (ties to the LAST index) must not survive the quantised cases."""
    caught = sum(not np.array_equal(R.match_scores(s, thr)[0], R.match_scores(s, thr, mutant=True)[0]) for s, thr in quantised_cases())
    assert caught > 40


@pytest.mark.parametrize("case", R.list_cases(), ids=lambda c: c[0])
def test_restatement_list_cases(case):
    _, matches, n_ref, n_cur, expected = case
    idx, st = R.match_list(matches, n_ref, n_cur)
    assert idx.tolist() == expected
    assert st.tolist() == [R.TRACKED if j >= 0 else R.LARGE_RESIDUAL for j in expected]


def test_restatement_list_against_python_loop():
    rng = np.random.default_rng(9)
    for _ in range(50):
        n_ref, n_cur, k = int(rng.integers(1, 12)), int(rng.integers(0, 12)), int(rng.integers(0, 40))
        m = rng.integers(-3, 14, size=(k, 2)).astype(np.int64)
        want = [-1] * n_ref
        for a, b in m.tolist():
            if 0 <= a < min(n_ref, n_cur) and 0 <= b < n_cur:
                want[a] = b
        assert R.match_list(m, n_ref, n_cur)[0].tolist() == want


def test_restatement_fill():
    uv = np.float32([[10, 11], [20, 21], [30, 31]])
    # n_ref < n_cur: the tail of matched_uv stays cur_uv
    assert R.fill([2, -1], uv).tolist() == [[30, 31], [20, 21], [30, 31]]
    # n_ref > n_cur: rows 3, 4 are matched but have no entry — nothing written, nothing read out of range
    assert R.fill([1, -1, 0, 2, 0], uv).tolist() == [[20, 21], [20, 21], [10, 11]]
    assert R.fill([], uv).tolist() == uv.tolist()
    assert R.fill([0, 0], np.zeros((0, 2), np.float32)).shape == (0, 2)


# ---- the launch plan ----

def plan(cases):
    assert os.path.exists(PLAN_EXE), "host layer not built (python -c 'import __graft_entry__ as g; g.build()')"
    text = "\n".join("nn " + " ".join(str(c[f]) for f in ("batch", "n_ref", "n_cur", "row_stride", "batch_stride", "aligned16")) for c in cases) + "\n"
    r = subprocess.run([PLAN_EXE], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        d = {}
        for kv in line.split():
            k, v = kv.split("=")
            d[k] = tuple(int(t) for t in v.split("x")) if re.fullmatch(r"\d+x\d+", v) else int(v)
        out.append(d)
    assert len(out) == len(cases)
    return out


def cdiv(a, b):
    return -(-a // b)


def test_nn_match_plan_properties():
    sizes = (1, 2, 15, 16, 17, 255, 256, 257, 300, 1023, 1024, 2049, 4096, 100000)
    cases = []
    for B, n_ref, n_cur in itertools.product((1, 3, 64), sizes, sizes):
        for pad, aligned in ((0, 1), (1, 1), (4, 1), (0, 0)):
            rs = n_cur + pad
            cases.append(dict(batch=B, n_ref=n_ref, n_cur=n_cur, row_stride=rs, batch_stride=(n_ref + (1 if pad else 0)) * rs, aligned16=aligned))
    seen_rows = set()
    for c, p in zip(cases, plan(cases)):
        what = f"{c} -> {p}"
        B, n_ref, n_cur = c["batch"], c["n_ref"], c["n_cur"]
        assert p["ok"] == 1, what
        assert p["vec4"] == int(c["aligned16"] == 1 and c["row_stride"] % 4 == 0 and c["batch_stride"] % 4 == 0), what
        # the tile: 256 columns, 16 .. 128 rows in whole rounds of the workgroup's four waves x four loads
        assert p["tile_cols"] == 256 and p["tile_rows"] in (16, 32, 64, 128), what
        seen_rows.add(p["tile_rows"])
        # every row and every column in exactly one tile: the tiles partition [0, n_ref) x [0, n_cur) with no empty tile
        assert p["row_tiles"] == cdiv(n_ref, p["tile_rows"]) and p["col_tiles"] == cdiv(n_cur, 256), what
        assert (p["row_tiles"] - 1) * p["tile_rows"] < n_ref <= p["row_tiles"] * p["tile_rows"], what
        assert (p["col_tiles"] - 1) * 256 < n_cur <= p["col_tiles"] * 256, what
        assert p["grid"] == (p["row_tiles"] * p["col_tiles"], B) and p["block"] == (256, 1), what
        # taller tiles only while they leave the chip about four workgroups per CU
        if p["tile_rows"] > 16:
            assert B * p["col_tiles"] * p["row_tiles"] >= 1024, what
        if p["tile_rows"] < 128:
            assert B * p["col_tiles"] * cdiv(n_ref, 2 * p["tile_rows"]) < 1024, what
        # grid limits and the workspace bound
        assert 1 <= p["grid"][0] < 2 ** 31 and 1 <= p["grid"][1] <= 65535, what
        assert p["key_count"] == B * (n_ref + n_cur) + 1, what
        assert p["epilogue_grid"] == (cdiv(B * n_ref, 256), 1), what
    assert seen_rows == {16, 32, 64, 128}


def test_nn_match_plan_refuses_what_does_not_fit():
    base = dict(row_stride=8, batch_stride=64, aligned16=1)
    p = plan([dict(base, batch=65536, n_ref=2, n_cur=2), dict(base, batch=65535, n_ref=2, n_cur=2), dict(base, batch=1, n_ref=2 ** 30, n_cur=2 ** 30),
              dict(base, batch=1, n_ref=2 ** 30, n_cur=2 ** 30 - 1), dict(base, batch=0, n_ref=2, n_cur=2), dict(base, batch=1, n_ref=0, n_cur=2),
              dict(base, batch=1, n_ref=2, n_cur=0), dict(base, batch=3, n_ref=2 ** 29, n_cur=2 ** 29), dict(base, batch=1, n_ref=2 ** 31 - 258, n_cur=256)])
    # batch beyond grid.y; 2^31 key indices; 2^45 tiles; sizes below 1; batch * (n_ref + n_cur) = 3 * 2^30; the last key index, one column tile
    assert [q["ok"] for q in p] == [0, 1, 0, 0, 0, 0, 0, 0, 1]
    assert p[8]["grid"][0] == (2 ** 31 - 258 + 127) // 128 and p[8]["key_count"] == 2 ** 31 - 1


def test_nn_match_plan_pinned():
    base = dict(batch=1, aligned16=1)
    p = plan([dict(base, n_ref=300, n_cur=300, row_stride=300, batch_stride=0),        # the reference's default size
              dict(base, n_ref=2048, n_cur=2048, row_stride=2049, batch_stride=0),     # LightGlue's [:, :-1, :-1] view: 4-byte loads
              dict(base, n_ref=4096, n_cur=4096, row_stride=4096, batch_stride=0)])
    assert (p[0]["tile_rows"], p[0]["grid"], p[0]["vec4"], p[0]["key_count"]) == (16, (38, 1), 1, 601)
    assert (p[1]["tile_rows"], p[1]["grid"], p[1]["vec4"]) == (16, (1024, 1), 0)
    assert (p[2]["tile_rows"], p[2]["grid"], p[2]["vec4"], p[2]["epilogue_grid"]) == (64, (1024, 1), 1, (16, 1))


# ---- ABI surface ----

def test_nn_symbols_in_header_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ftk.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ftk_[a-z_0-9]+)\s*\(", text))
    for name in NN_SYMBOLS:
        assert name in declared, name
    assert "#define FTK_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "ftk.h")).read()  # functions are only added
    from feature_tracker_amd import _native
    for name in NN_SYMBOLS:
        assert name in _native.EXPORTS, name
    if os.path.exists(_native.LIB_PATH):
        lib = _native.lib()
        for name in NN_SYMBOLS:
            assert hasattr(lib, name), name


def test_public_class_is_exported():
    import feature_tracker_amd as F
    m = F.NNFeatureMatcher()
    o = m.options()
    assert (o.kMaxNumberOfMatches, o.kMinValidMatchScore, o.kModelType) == (300, -3.0, 0)  # nn_feature_matcher.h:23-27
    assert "NNFeatureMatcher" in F.__all__


def test_product_does_not_import_the_restatement():
    pkg = os.path.join(ROOT, "feature_tracker_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".hpp")) or f == "Makefile":
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "nn_match_ref" not in text and "nmr_" not in text, os.path.join(dirpath, f)


def test_cpp_class_without_an_inference_function_returns_false():
    """Match without SetInference returns false before any device use, as the reference does with a null session (:94)."""
    exe = os.path.join(ROOT, "feature_tracker_amd", "host", "build", "nn_match_cli")
    assert os.path.exists(exe), "host layer not built"
    env = dict(os.environ, FTK_NO_WARMUP="1")
    r = subprocess.run([exe, "none", "3", "3"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 1 and r.stdout.strip() == "ok 0", r.stdout + r.stderr
    # ... and an empty reference set returns false first (:92)
    r = subprocess.run([exe, "none", "0", "3"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 1 and r.stdout.strip() == "ok 0", r.stdout + r.stderr
