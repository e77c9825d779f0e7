"""The cosine matcher at every descriptor width, the part that needs no device: that the cases of tests/cosine_width_cases.py reach what
tests/test_cosine_widths_gpu.py means them to reach (plans, branches of the exact dot product, conditions on the inputs), that the
oracle they are compared with is itself right at these widths (against float64), that the comparison would notice (mutants), and
that the shortlist's error budget, as a function of the width, stays under the margin the plan hands the kernels.

The budget (float_matcher_kernels.hip states it; budget() below evaluates it)
---------------------------------------------------------------------------
The shortlist keeps, per reference row, every candidate whose approximate cosine lies within 2 * margin of the row's approximate
maximum; the deciding candidate is among them if |c~ - c| <= margin for every regular pair, where c = 1 - 2 d is the cosine of the
distance d as the exact side computes it.  With u = 2^-24, a = x / fl-norm(x), b = y / fl-norm(y) (|a|, |b| <= 1 + dn,
dn = (dim / 16 + 5) u the norm's own relative error, which both sides share):

  fp16 copies   each component is off by at most r |a_k| (normal; r = 2^-11 + 2^-22 with the fp32 scaling before it) or by
                s = 2^-25 + 2^-37 (below 2^-14: half a subnormal step), so by Cauchy-Schwarz the copy is off by at most
                h = r |a| + s sqrt(dim) in length, and the cosine by 2 h (1 + dn) + h^2;
  accumulation  v_mfma_f32_32x32x16_f16 forms exact products; how it rounds inside is not specified, so every addend of every
                instruction (16 products and the incoming accumulator) is charged one unit in the last place of the running sum,
                truncated: (17 / 16) dim_pad 2^-23 of sum |a^ b^| <= (1 + dn + h)^2;
  exact side    Eigen's order puts every product through at most dim / 8 + 7 roundings (one product, dim / 8 - 1 adds per packet
                lane, three to combine, three of the tail), the two divisions add 2 u, the final 0.5 - 0.5 c half an ulp of
                d < 1, i.e. u on the cosine: (dim / 8 + 10) u (1 + dn)^2;
  index bits    the register-stationary kernel overwrites 5 mantissa bits of a score of at most 1 + ...: 31 * 2^-23.

The oracle against float64
--------------------------
d_fl = d_64 + e with |e| <= E(dim) = (dim / 8 + 9.5) u: the dot product as above (dim / 8 + 7) u sum |a_k b_k| <= (dim / 8 + 7) u, the
two norms half of that plus the square root each, (dim / 8 + 9) u |c| together, two divisions 2 u, all halved by the 0.5, and half
an ulp of the final subtraction.  The candidate the oracle picks minimises d_fl, so its d_64 is at most 2 E above the float64
minimum (1 % added for the second-order terms).  The derived bound is used as it stands; it needed no padding."""
import functools
import math

import numpy as np
import pytest

from tests import cosine_width_cases as W
from tests.test_match_plan_cpu import plan

U = 2.0 ** -24
MUTANT_DIMS = (5, 160, 321, 4096)


# ---- what the widths reach ----

def width_plans(**overrides):
    return plan("cosine", [dict(n_ref=W.N_REF, n_cur=W.N_CUR, dim=d, **overrides) for d in W.WIDTHS])


def test_the_widths_and_the_shape():
    assert W.WIDTHS[:40] == tuple(range(1, 41)) and len(set(W.WIDTHS)) == len(W.WIDTHS) == 68
    assert set(W.WIDTHS[40:]) == {63, 64, 65, 100, 127, 128, 129, 130, 136, 160, 191, 192, 193, 255, 256, 257, 264, 319, 320, 321, 511, 512, 513, 1000,
                                  1021, 2048, 4095, 4096}
    assert (W.N_REF, W.N_CUR, W.WINDOW) == (130, 200, (60, 45))


@pytest.mark.parametrize("nearby", [0, 1])
def test_plan_reach(nearby):
    """Every width plans the form the GPU tests are there for: register-stationary with 4, 8, 12 and 16 K steps up to 256 (12 exactly
    for 129 .. 192), the chunked pair with dim_pad / 64 chunks above (5, 8, 16, 32 and 64 among them), the packet-wide prep exactly
    for dim % 8 == 0; 64, 128 and 256 plan the one-launch form unless it is switched off."""
    default, launches = width_plans(nearby=nearby), width_plans(nearby=nearby, small=0)
    ksteps, chunks = {}, {}
    for dim, p, q in zip(W.WIDTHS, default, launches):
        what = f"{dim}: {q}"
        assert p["dim_pad"] == q["dim_pad"] == W.dim_pad(dim), what
        assert (p["form"] == "small") == (dim in (64, 128, 256)), what
        if p["form"] != "small":
            assert p["form"] == q["form"] and p["grid"] == q["grid"], what
        assert q["packet_prep"] == int(dim % 8 == 0), what
        assert q["n_ref_pad"] == (512 if dim <= 256 else 256) and q["n_cur_pad"] == 256, what  # ragged tails in every row group
        if dim <= 256:
            assert q["form"] == "register_stationary", what
            ksteps.setdefault(q["dim_pad"] // 16, []).append(dim)
        else:
            assert q["form"] == "chunked" and q["grid"] == (2, 2), what  # two row tiles, two candidate tiles of 128
            chunks.setdefault(q["dim_pad"] // 64, []).append(dim)
        assert float(q["margin"]) == pytest.approx(W.plan_margin(dim), rel=1e-6), what
    assert sorted(ksteps) == [4, 8, 12, 16]
    assert ksteps[12] == [d for d in W.WIDTHS if 129 <= d <= 192] and len(ksteps[12]) >= 6
    assert {5, 8, 16, 32, 64} <= set(chunks) and min(chunks) == 5 and max(chunks) == 64


def test_forced_forms_reach():
    """test_wide_forms_at_forced_splits: FTK_COSINE_CHUNKED=1 at 160 and 192 runs the chunked pair with 3 chunks; FTK_COSINE_SPLITS 1, 2
    and 5 give that many workgroups per row group, capped by the tiles there are."""
    for dim in (160, 192):
        p, = plan("cosine", [dict(n_ref=W.N_REF, n_cur=W.N_CUR, dim=dim, chunked=1)])
        assert p["form"] == "chunked" and p["dim_pad"] // 64 == 3 and float(p["margin"]) == pytest.approx(W.K_MARGIN, rel=1e-6)
    for dim in (160, 192, 320, 1000, 4096):
        tiles = 4 if dim <= 256 else 2
        for splits in (1, 2, 5):
            p, = plan("cosine", [dict(n_ref=W.N_REF, n_cur=W.N_CUR, dim=dim, splits=splits)])
            assert p["splits"] == min(splits, tiles), (dim, splits, p)


def test_tile_list_cap_reach():
    """test_more_cur_tiles_than_the_tile_list_holds: 65 600 candidates are 1 025 tiles of 64, one more than kRrListCap; 65 536 are 1 024."""
    for n_cur, tiles in ((65600, 1025), (65536, 1024)):
        p, = plan("cosine", [dict(n_ref=64, n_cur=n_cur, dim=64, nearby=1, small=0)])
        assert p["form"] == "register_stationary" and p["n_cur_pad"] // 64 == tiles and p["use_tile_box"] == 1, p
        assert p["ws_bytes"] < 100 << 20, p


def test_eigen_dot_branch_coverage():
    """WIDTHS takes every combination of eigen_dot_octet's branches that a size in 1 .. 4096 can take, every tail length beside each of
    them, and the main loop (index 8 ..) not at all, once and many times."""
    reachable = {W.eigen_dot_branches(d) for d in range(1, 4097)}
    assert reachable == {(True, False, False, True), (False, True, True, False), (False, True, True, True), (False, False, False, False),
                         (False, False, False, True), (False, False, True, False), (False, False, True, True)}
    assert {W.eigen_dot_branches(d) for d in W.WIDTHS} == reachable
    with_tail = lambda dims: {W.eigen_dot_branches(d) + (d % 4, min(d // 8, 3)) for d in dims}
    assert with_tail(W.WIDTHS) == with_tail(range(1, 4097))
    assert {d % 8 for d in W.WIDTHS if d > 8} == set(range(8))


# ---- conditions on the inputs (float64; not measurements of the code under test) ----

@pytest.mark.parametrize("dim", W.WIDTHS)
def test_near_ties_condition(dim, oracle):
    """Every clustered row has at least 10 candidates within kMargin / 4 of its float64 minimum, the group lies where it is said to
    lie, and at MUTANT_DIMS and beyond 8 components some row's winner is a duplicated candidate (the lower index wins)."""
    c = W.near_ties(dim)
    near_tie_conditions(c, oracle, dim, need_duplicate=dim >= 8)


def near_tie_conditions(c, oracle, dim, need_duplicate):
    d64 = W.distances64(c.ref, c.cur)
    rows = np.array(W.TIE_ROWS)
    assert rows.size == 40 and len(W.TIE_SLOTS) == 30
    assert min(W.TIE_SLOTS) < 64 <= max(s for s in W.TIE_SLOTS if s < 100) and min(s for s in W.TIE_SLOTS if s > 100) < 128 <= max(W.TIE_SLOTS)
    close = d64[rows] <= d64[rows].min(axis=1, keepdims=True) + W.K_MARGIN / 4
    assert (close.sum(axis=1) >= 10).all(), (dim, close.sum(axis=1).min())
    later, earlier = W.TIE_SLOTS[W.DUP_LATER[0]], W.TIE_SLOTS[W.DUP_EARLIER[0]]
    assert np.array_equal(c.cur[W.DUP_LATER[1]], c.cur[later]) and W.DUP_LATER[1] > later
    assert np.array_equal(c.cur[W.DUP_EARLIER[1]], c.cur[earlier]) and W.DUP_EARLIER[1] < earlier
    _, idx = oracle.match_float(c.ref, c.cur, 0.6)
    if need_duplicate:
        assert (idx[rows] == later).any() or (idx[rows] == W.DUP_EARLIER[1]).any(), dim
    assert not (idx == W.DUP_LATER[1]).any() and not (idx == earlier).any(), dim  # the higher index of a pair of duplicates never wins
    inside = (np.abs(c.pred_uv[rows, None, :] - c.cur_uv[None, list(W.TIE_SLOTS), :]) <= np.float32(W.WINDOW)).all(axis=2)
    assert inside.any() and not inside.all(), dim  # the window cuts through the group


@pytest.mark.parametrize("dim", [d for d in W.WIDTHS if d >= W.HEAVY_TAIL_MIN_DIM])
def test_heavy_tail_condition(dim, oracle):
    """At least 30 % (in fact all but 8 per row) of the normalised components are below 2^-14: fp16 subnormals or zero; and the rows carry
    a near-tie group that meets the same conditions as near_ties."""
    c = W.heavy_tail(dim)
    for x in (c.ref, c.cur):
        unit = np.abs(x.astype(np.float64)) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
        assert (unit < 2.0 ** -14).mean() >= 0.30
        assert ((unit < 2.0 ** -14).sum(axis=1) >= dim - 8 - 30).all() and (unit.max(axis=1) > 0.2).all()
    near_tie_conditions(c, oracle, dim, need_duplicate=True)


@pytest.mark.parametrize("dim", [160, 320, 4096])
def test_overflow_and_irregular_conditions(dim):
    c = W.overflow(dim)
    d64 = W.distances64(c.ref, c.cur)
    assert c.cur.shape[0] == 1200
    assert ((d64 <= d64.min(axis=1, keepdims=True) + W.K_MARGIN).sum(axis=1) > W.CAND_CAP).all()
    a, b = W.irregular(dim), W.irregular(dim, beyond_cap=True)
    assert W.irregular_rows(a.ref).sum() == 5 and W.irregular_rows(a.cur).sum() == 4 <= W.IRREGULAR_CAP
    assert W.irregular_rows(b.cur).sum() == 4 + 70 > W.IRREGULAR_CAP


# ---- the oracle against float64 ----

def oracle_gap_bound(dim):
    return 2.0 * 1.01 * (math.ceil(dim / 8) + 9.5) * U


def builders(dim):
    yield "planted", W.planted(dim)
    yield "near_ties", W.near_ties(dim)
    if dim >= W.HEAVY_TAIL_MIN_DIM:
        yield "heavy_tail", W.heavy_tail(dim)
    yield "overflow", W.overflow(dim)
    c = W.irregular(dim)  # the regular rows and candidates of it: on the others float64 and fp32 differ by design (overflow, 0 / 0)
    yield "irregular", W.Case(c.ref[~W.irregular_rows(c.ref)], c.cur[~W.irregular_rows(c.cur)], None, None)


@pytest.mark.parametrize("dim", W.WIDTHS)
def test_oracle_against_float64(dim, oracle):
    """The candidate oracle.match_float picks (threshold above every distance, so every row picks) is, in float64, no further from
    the float64 minimum than oracle_gap_bound(dim) — the module docstring derives it."""
    for name, c in builders(dim):
        ok, idx = oracle.match_float(c.ref, c.cur, 1.5)
        assert ok and (idx >= 0).all(), (name, dim)
        d64 = W.distances64(c.ref, c.cur)
        gap = d64[np.arange(idx.size), idx] - d64.min(axis=1)
        assert gap.max() <= oracle_gap_bound(dim), (name, dim, gap.max(), oracle_gap_bound(dim))


# ---- mutants of the oracle call: the GPU comparison has teeth at the new widths ----

def fp16_copies(x, dim):
    """What the contraction sees: the unit-length fp16 copy of each row, zero-padded to dim_pad."""
    unit = (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True).astype(np.float32)).astype(np.float16).astype(np.float32)
    return np.pad(unit, ((0, 0), (0, W.dim_pad(dim) - dim)))


@pytest.mark.parametrize("dim", MUTANT_DIMS)
def test_mutants_change_an_index(dim, oracle):
    c = W.near_ties(dim)
    thr = 0.6
    _, want = oracle.match_float(c.ref, c.cur, thr)
    n = c.cur.shape[0]
    # the highest index on ties
    _, rev = oracle.match_float(c.ref, c.cur[::-1], thr)
    highest = np.where(rev >= 0, n - 1 - rev, rev)
    assert (highest != want).any()
    # '<=' instead of '<' at the threshold: a threshold equal to a row's minimum matches nothing under '<' and that row under '<='
    row = W.TIE_ROWS[W.DUP_EARLIER[0]]
    d_min = oracle.cosine_distance(c.ref[row], c.cur[want[row]])
    _, strict = oracle.match_float(c.ref, c.cur, float(d_min))
    _, loose = oracle.match_float(c.ref, c.cur, float(np.nextafter(d_min, np.float32(2.0))))
    assert strict[row] == -1 and loose[row] == want[row] and (strict != loose).any()
    # descriptors truncated to dim - 1
    _, cut = oracle.match_float(c.ref[:, :dim - 1], c.cur[:, :dim - 1], thr)
    assert (cut != want).any()
    # deciding on the zero-padded unit-length fp16 copies instead of the fp32 rows
    _, approx = oracle.match_float(fp16_copies(c.ref, dim), fp16_copies(c.cur, dim), thr)
    assert (approx != want).any()


# ---- the error budget at every accepted width ----

def budget(dim, dim_pad, register_stationary):
    """Bound on |c~ - c| (cosine domain) of a regular pair; the terms are those of the module docstring, in its order."""
    dn = (dim / 16 + 5) * U
    r, s = 2.0 ** -11 + 2.0 ** -22, 2.0 ** -25 + 2.0 ** -37
    h = r * (1 + dn) + s * math.sqrt(dim)
    fp16 = 2 * h * (1 + dn) + h * h
    m = (17 / 16) * dim_pad * 2.0 ** -23
    accumulation = m / (1 - m) * (1 + dn + h) ** 2
    exact = (dim / 8 + 10) * U * (1 + dn) ** 2
    index_bits = 31 * 2.0 ** -23 if register_stationary else 0.0
    return fp16 + accumulation + exact + index_bits


def test_budget_stays_under_the_plans_margin():
    """2 eps < margin, i.e. budget < margin on the cosine, with at least a quarter of the margin to spare at EVERY accepted width and
    with the margin the plan CLI prints (so the C++ and this file cannot drift apart); the constant 1.5e-3 alone is proven up to 3840
    components and has a quarter to spare up to 1024 — the reason the plan's margin grows."""
    dims = sorted(set(range(1, 4097, 1)))
    plans = plan("cosine", [dict(n_ref=W.N_REF, n_cur=W.N_CUR, dim=d, small=0) for d in dims])
    worst = 0.0
    for dim, p in zip(dims, plans):
        margin = float(p["margin"])
        assert margin == pytest.approx(W.plan_margin(dim), rel=1e-6)
        if p["dim_pad"] <= 256:
            assert margin == float(np.float32(W.K_MARGIN)) or margin == pytest.approx(W.K_MARGIN, rel=1e-7)
        b = budget(dim, p["dim_pad"], p["form"] == "register_stationary")
        assert b <= 0.75 * margin, (dim, b, margin)
        worst = max(worst, b / margin)
    assert 0.70 < worst <= 0.75  # the growth is not lavish either
    for dim in (256, 1024, 4096):
        assert budget(dim, dim, dim <= 256) / 2 < W.plan_margin(dim) / 2  # eps on the distance against half the margin
    # the constant margin of the narrow widths, had it been kept for all: where the proof ends and where its slack does
    constant = lambda dim: budget(dim, W.dim_pad(dim), False) / W.K_MARGIN
    assert constant(3840) < 1.0 < constant(3841) and constant(4096) > 1.0
    assert constant(1024) <= 0.75 < constant(1025)


@functools.lru_cache(maxsize=None)
def _chunked_at_256():
    return plan("cosine", [dict(n_ref=W.N_REF, n_cur=W.N_CUR, dim=256, small=0, chunked=1)])[0]


def test_forced_chunked_keeps_the_narrow_margin():
    """FTK_COSINE_CHUNKED=1 up to 256 runs the chunked pair under the constant margin; its budget has no index bits."""
    p = _chunked_at_256()
    assert p["form"] == "chunked" and budget(256, 256, False) <= 0.75 * float(p["margin"])
