"""The scalar restatement of LightGlue's assignment head (tests/match_assignment_ref.c) pinned without a device: known
answers by hand, upstream's formula in torch float64, the mutual-best matches both give, and five mutants.

Measured here against float64 at the GPU tests' shapes (match_assignment_ref.SHAPES): the worst absolute deviation of an entry is 2.2e-6
without weights (scores down to -27) and 8.8e-6 with weights (scores down to -79, where one float32 ulp is 7.6e-6); both are asserted
at four times that, the project's margin for exp_c-built quantities.  log_c's worst error against float64 log over [1, 4096] is 0.77 ulp,
asserted below 1 ulp (the bound of the fdlibm kernel it restates).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import match_assignment_ref as R  # noqa: E402

TOL = {False: 4 * 2.2e-6, True: 4 * 8.8e-6}
LOG_C_ULP = 1.0
MAX_AMBIGUOUS = 0.02


def upstream_float64(a, b, weights=None, bias=None, count0=None, count1=None):
    """MatchAssignment.forward of upstream LightGlue on the valid block, in torch float64: linear, / d ** .25, matmul, two log_softmax,
    logsigmoid; -inf in every invalid row and column."""
    F = torch.nn.functional
    a, b = torch.tensor(np.asarray(a), dtype=torch.float64), torch.tensor(np.asarray(b), dtype=torch.float64)
    (m, d), n = a.shape, b.shape[0]
    n0 = m if count0 is None else min(max(count0, 0), m)
    n1 = n if count1 is None else min(max(count1, 0), n)
    out = torch.full((m + 1, n + 1), -float("inf"), dtype=torch.float64)
    out[m, n] = 0.0
    if weights is not None:
        w, bb = torch.tensor(weights, dtype=torch.float64), torch.tensor(bias, dtype=torch.float64)
        md0, md1 = F.linear(a, w[:d], bb[:d]) / d ** .25, F.linear(b, w[:d], bb[:d]) / d ** .25
        z0, z1 = F.linear(a, w[d:], bb[d:])[:, 0], F.linear(b, w[d:], bb[d:])[:, 0]
        out[:n0, n] = F.logsigmoid(-z0[:n0])
        out[m, :n1] = F.logsigmoid(-z1[:n1])
    else:
        md0, md1 = a * R.default_scale(d), b * R.default_scale(d)
    if n0 and n1:
        sim = (md0 @ md1.T)[:n0, :n1]
        v = F.log_softmax(sim, 1) + F.log_softmax(sim, 0)
        if weights is not None:
            v = v + F.logsigmoid(z0[:n0])[:, None] + F.logsigmoid(z1[:n1])[None, :]
        out[:n0, :n1] = v
    return out.numpy()


@functools.lru_cache(maxsize=None)
def both(shape, with_weights):
    a, b, kw = R.case(shape, with_weights)
    return R.assign(a, b, **kw), upstream_float64(a, b, kw.get("weights"), kw.get("bias"))


def worst_deviation(got, want):
    finite = np.isfinite(want)
    assert np.array_equal(got[~finite].astype(np.float64), want[~finite])
    return float(np.abs(got[finite].astype(np.float64) - want[finite]).max()) if finite.any() else 0.0


# ---- known answers -------------------------------------------------------------------------------------------------------------------

def test_one_pair_without_weights_is_exactly_zero():
    for value, d in ((0.75, 1), (-3.0, 5), (1e3, 64)):
        s = R.assign(np.full((1, d), value, np.float32), np.full((1, d), value, np.float32))
        # a single entry is its own row and column maximum: sim - (sim + log_c(1)) on both axes
        assert s.shape == (2, 2) and s[0, 0] == 0.0 and not np.signbit(s[0, 0])
        assert s[0, 1] == -np.inf and s[1, 0] == -np.inf and s[1, 1] == 0.0 and not np.signbit(s[1, 1])


def test_one_pair_with_weights_is_the_certainty_term():
    d = 3
    fw, fb = np.float32([[1, 0, 0], [0, 2, 0], [0, 0, -1]]), np.float32([0.5, 0, -0.25])
    mw, mb = np.float32([[0.5, -1.0, 2.0]]), np.float32([0.125])
    x0, x1 = np.float32([[1, 2, 3]]), np.float32([[-1, 0.5, 0.25]])
    z0, z1 = np.float32(0.125 + 0.5 - 2.0 + 6.0), np.float32(0.125 - 0.5 - 0.5 + 0.5)  # exact in float32, any order
    w, b = R.pack(fw, fb, mw, mb)
    s = R.assign(x0, x1, weights=w, bias=b)
    assert s[0, 0] == np.float32(R.ls(z0) + R.ls(z1))
    assert s[0, 1] == R.ls(-z0) and s[1, 0] == R.ls(-z1) and s[1, 1] == 0.0
    assert abs(float(R.ls(z0)) - float(torch.nn.functional.logsigmoid(torch.tensor(float(z0), dtype=torch.float64)))) < 1e-6
    assert R.ls(0.0) == np.float32(-np.log(2.0)) and np.isnan(R.ls(np.nan)) and R.ls(-200.0) == np.float32(-200.0)


def test_identical_descriptors_give_equal_entries():
    x = np.tile(np.linspace(-1, 1, 16, dtype=np.float32), (64, 1))
    s = R.assign(x, x)
    block = s[:64, :64]
    assert (block.view(np.uint32) == block.view(np.uint32)[0, 0]).all()
    # 64 equal terms: every partial holds exactly 1, the butterfly gives exactly 64
    assert block[0, 0] == np.float32(-2.0) * R.log_c([64.0])[0]
    assert abs(float(block[0, 0]) + 2 * np.log(64.0)) < 4e-6


def test_zero_count_leaves_only_the_corner():
    a, b, kw = R.case(R.SHAPES[4], False)
    s = R.assign(a, b, count0=0)
    corner = np.zeros_like(s, bool)
    corner[-1, -1] = True
    assert (s[~corner] == -np.inf).all() and s[-1, -1] == 0.0
    # with weights the columns are still valid: rule 5 gives their dustbin entries, rule 6 takes every row
    a, b, kw = R.case(R.SHAPES[4], True)
    s, full = R.assign(a, b, count0=0, **kw), R.assign(a, b, **kw)
    assert (s[:-1] == -np.inf).all() and R.same(s[-1], full[-1]) and np.isfinite(s[-1]).all()
    s = R.assign(a, b, count0=0, count1=0, **kw)
    assert (s[~corner] == -np.inf).all() and s[-1, -1] == 0.0


def test_counts_clamp_and_cut_the_valid_block():
    a, b, kw = R.case(R.SHAPES[4], True)
    m, n = a.shape[0], b.shape[0]
    assert R.same(R.assign(a, b, count0=m + 7, count1=n + 1, **kw), R.assign(a, b, **kw))
    assert R.same(R.assign(a, b, count0=-3, **kw), R.assign(a, b, count0=0, **kw))
    cut = R.assign(a, b, count0=20, count1=33, **kw)
    # the valid block is the assignment of the first 20 and 33 descriptors alone
    small = R.assign(a[:20], b[:33], **kw)
    assert R.same(cut[:20, :33], small[:20, :33]) and R.same(cut[:20, n], small[:20, 33]) and R.same(cut[m, :33], small[20, :33])
    assert (cut[20:m] == -np.inf).all() and (cut[:, 33:n] == -np.inf).all() and cut[m, n] == 0.0


def test_strided_rows_leave_the_padding():
    a, b, kw = R.case(R.SHAPES[2], True)
    s = R.assign(a, b, row_stride=40, **kw)
    assert R.same(s, R.assign(a, b, **kw)) and (s.base[:, b.shape[0] + 1:] == R.SENTINEL).all()


def test_log_c_against_float64():
    x = np.concatenate([np.linspace(1, 4096, 400001), 1 + np.linspace(0, 1, 200001), 2.0 ** np.arange(0, 13)]).astype(np.float32)
    got, want = R.log_c(x).astype(np.float64), np.log(x.astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    keep = want != 0
    worst = float((np.abs(got - want)[keep] / ulp[keep]).max())
    print(f"log_c: worst error {worst:.3f} ulp over [1, 4096]")
    assert worst < LOG_C_ULP
    one = R.log_c([1.0])
    assert one[0] == 0.0 and not np.signbit(one[0]) and np.isnan(R.log_c([np.nan])[0])
    assert (np.diff(R.log_c(np.arange(1, 4097, dtype=np.float32))) > 0).all()


# ---- against upstream's formula in float64 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_weights", [False, True], ids=["without_weights", "with_weights"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(str(v) for v in s[:3]))
def test_restatement_against_float64(shape, with_weights):
    got, want = both(shape, with_weights)
    worst = worst_deviation(got, want)
    print(f"{shape[:3]} weights={with_weights}: worst |restatement - float64| = {worst:.3g}")
    assert worst <= TOL[with_weights]


@pytest.mark.parametrize("with_weights", [False, True], ids=["without_weights", "with_weights"])
def test_counts_against_float64(with_weights):
    shape = R.SHAPES[7]
    a, b, kw = R.case(shape, with_weights)
    for c0, c1 in ((0, None), (1, 1), (65, 64), (130, 77), (500, 1)):
        got = R.assign(a, b, count0=c0, count1=c1, **kw)
        assert worst_deviation(got, upstream_float64(a, b, kw.get("weights"), kw.get("bias"), c0, c1)) <= TOL[with_weights]


def mutual_best(block):
    """match[i] = j where j is row i's best column and i column j's best row, else -1 (first index on ties, as argmax)."""
    rows, cols = block.argmax(1), block.argmax(0)
    return np.where(cols[rows] == np.arange(block.shape[0]), rows, -1)


def near_tie(block, tol):
    """Per row: its two best entries lie within tol, or those of its best column do."""
    def two_best_close(x):
        if x.shape[1] < 2:
            return np.zeros(x.shape[0], bool)
        top = np.sort(x, axis=1)[:, -2:]
        return top[:, 1] - top[:, 0] <= tol
    return two_best_close(block) | two_best_close(block.T)[block.argmax(1)]


@pytest.mark.parametrize("with_weights", [False, True], ids=["without_weights", "with_weights"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(str(v) for v in s[:3]))
def test_mutual_best_matches_equal_float64s(shape, with_weights):
    got, want = both(shape, with_weights)
    m, n = shape[:2]
    ties = near_tie(want[:m, :n], TOL[with_weights])
    assert ties.mean() <= MAX_AMBIGUOUS, "the seed leaves float64 itself ambiguous in too many rows"
    differ = mutual_best(got[:m, :n].astype(np.float64)) != mutual_best(want[:m, :n])
    assert not (differ & ~ties).any() and differ.mean() <= MAX_AMBIGUOUS
    if min(m, n) >= 31 and shape[2] >= 64:
        assert (mutual_best(want[:m, :n]) >= 0).sum() >= 0.8 * min(m, n)  # the planted pairs are found: the comparison is not vacuous


# ---- mutants -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.MUTANTS))
def test_each_mutant_is_caught(name):
    shape, with_weights = R.SHAPES[7], True
    a, b, kw = R.case(shape, with_weights)
    count1 = 65 if name == "invalid_columns_in_a_rows_normaliser" else None
    want = upstream_float64(a, b, kw["weights"], kw["bias"], None, count1)
    assert worst_deviation(R.assign(a, b, count1=count1, **kw), want) <= TOL[with_weights]
    mutant = R.assign(a, b, count1=count1, variant=R.MUTANTS[name], **kw)
    finite = np.isfinite(want)
    assert np.abs(mutant[finite].astype(np.float64) - want[finite]).max() > 1000 * TOL[with_weights]


@pytest.mark.parametrize("name", ["column_softmax_left_out", "scale_on_one_side_only", "invalid_columns_in_a_rows_normaliser"])
def test_each_mutant_without_weights_is_caught(name):
    a, b, kw = R.case(R.SHAPES[7], False)
    count1 = 65 if name == "invalid_columns_in_a_rows_normaliser" else None
    want = upstream_float64(a, b, None, None, None, count1)
    mutant = R.assign(a, b, count1=count1, variant=R.MUTANTS[name])
    finite = np.isfinite(want)
    assert np.abs(mutant[finite].astype(np.float64) - want[finite]).max() > 1000 * TOL[False]
