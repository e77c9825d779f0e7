"""The scalar restatement of LightGlue's adaptive depth and width (tests/lightglue_adaptive_ref.c) on the CPU: known
answers steered through the tests' own weights, the float64 pin of conf and mt, decisions that no rounding can flip, and mutants that
each change some output of some case."""
import functools

import numpy as np
import pytest

from tests import lightglue_adaptive_ref as R
from tests import transformer_ref as T

SHAPE = R.SHAPES[2]      # 65 x 130, D = 64, four heads
SMALL = R.SHAPES[1]      # 33 x 31, D = 8
# |sigmoid_c(chain) - sigmoid(float64 dot product)| over test_conf_and_mt_against_float64's cases: measured worst 5.2e-7 (the chain's
# rounding at D = 256 under a slope of 1 / 4); the bound is 4 x that
PIN = 2.1e-6


@functools.lru_cache(maxsize=None)
def _run(shape, steer, depth, width, min_keypoints=0, c0=None, c1=None, variant=R.CONTRACT):
    a, b, e0, e1, sd = R.case(shape, **dict(steer))
    return R.run(a, b, shape[3], e0, e1, sd, R.N_LAYERS, depth, width, min_keypoints, c0, c1, variant=variant)


def _steer(kwargs):
    return tuple(sorted(kwargs.items()))


def test_a_token_bias_of_plus_30_stops_at_layer_0():
    r = _run(SHAPE, _steer(R.STOP_AT_0[0]), 0.95, 0.99)
    assert (r.stopped, r.stop_layer, r.live0, r.live1) == (1, 0, 65, 130) and (r.layers0 == 1).all() and (r.layers1 == 1).all()
    assert np.array_equal(r.ind0, np.arange(65)) and np.isnan(r.conf[1]).all()  # nothing ran after the stop, nothing was pruned at it


def test_a_token_bias_of_minus_30_never_stops_and_keeps_every_row():
    r = _run(SHAPE, _steer(R.NEVER[0]), 0.95, 0.99)
    assert (r.stopped, r.stop_layer, r.live0, r.live1) == (0, 2, 65, 130) and (r.layers0 == 3).all()
    plain = _run(SHAPE, _steer(R.NEVER[0]), -1, -1)  # neither mechanism: the same outputs
    assert R.same_outputs(r, plain)


def test_a_matchability_bias_of_minus_30_prunes_the_side_above_the_minimum_only():
    steer = _steer(dict(token_bias=(30.0, 30.0), match_bias=(-30.0, -30.0)))
    r = _run(SHAPE, steer, 1.0, 0.99, 100)  # confident tokens, and a depth_confidence no ratio exceeds: no stop
    assert (r.stopped, r.live0, r.live1) == (0, 65, 0) and (r.layers1 == 1).all() and (r.layers0 == 3).all()
    assert (r.match_index == -1).all() and (r.status == R.UNMATCHED).all()


def test_no_points_do_not_stop():
    r = _run(SMALL, _steer(R.STOP_AT_0[0]), 0.95, -1, 0, 0, 0)
    assert (r.stopped, r.stop_layer, r.live0, r.live1) == (0, 2, 0, 0) and (r.layers0 == 0).all() and (r.match_index == -1).all()


def test_counts_bound_the_layers_and_the_indices():
    r = _run(SHAPE, _steer(R.NEVER[0]), 0.95, 0.99, 0, 40, 101)
    assert (r.layers0[:40] == 3).all() and (r.layers0[40:] == 0).all() and (r.layers1[101:] == 0).all()
    assert (r.match_index[40:] == -1).all() and (r.match_index < 101).all()


def _float64_sigmoid(x, w, bias):
    z = x.astype(np.float64) @ w.astype(np.float64).ravel() + np.float64(bias)
    return 1.0 / (1.0 + np.exp(-z))


def _pruning_runs():
    for shape in (SMALL, SHAPE):
        for depth_on in (True, False):
            (a, b, e0, e1, sd), depth, width = R.prune_case(shape, depth_on)
            yield shape, sd, depth, width, R.run(a, b, shape[3], e0, e1, sd, R.N_LAYERS, depth, width)


def test_conf_and_mt_against_float64():
    rng = np.random.default_rng(11)
    worst = 0.0
    for d in (1, 5, 8, 64, 256):
        x, w = rng.standard_normal((200, d)).astype(np.float32), (3 * rng.standard_normal(d) / np.sqrt(d)).astype(np.float32)
        for bias in (-2.2, 0.0, 1.7):
            worst = max(worst, float(np.abs(R.confidence(x, w, bias) - _float64_sigmoid(x, w, bias)).max()))
    print("worst deviation of sigmoid_c of the chain from float64:", worst)
    assert worst <= PIN


def _float64_pass(shape, case, depth, width):
    """The pass with every decision made in float64: transformer_ref's layers on the live rows, conf and mt as float64 dot products of
    those descriptors, the stop ratio and the keep masks in float64, the compaction in numpy.  Returns (live0, live1, stop_layer, ind0,
    ind1, the least distance of a conf or mt from its threshold, the least distance of a stop ratio from depth_confidence)."""
    a, b, e0, e1, sd = case
    h, L, t = shape[3], R.N_LAYERS, R.thresholds(R.N_LAYERS).astype(np.float64)
    x, enc, ind = [np.array(a), np.array(b)], [np.array(e0), np.array(e1)], [np.arange(shape[0]), np.arange(shape[1])]
    points, stop_layer, margin, ratio_margin = shape[0] + shape[1], L - 1, np.inf, np.inf
    for i in range(L):
        x = list(T.layer(x[0], x[1], h, enc[0], enc[1], sd, f"transformers.{i}."))
        if i == L - 1:
            break
        conf = [_float64_sigmoid(v, sd[f"token_confidence.{i}.token.0.weight"], sd[f"token_confidence.{i}.token.0.bias"][0]) for v in x]
        mt = [_float64_sigmoid(v, sd[f"log_assignment.{i}.matchability.weight"], sd[f"log_assignment.{i}.matchability.bias"][0]) for v in x]
        bar = 1.0 - width
        margin = min([margin] + [float(np.abs(m - bar).min()) for m in mt])
        if depth > 0:
            margin = min([margin] + [float(np.abs(c - t[i]).min()) for c in conf])
            ratio = 1.0 - sum(int((c < t[i]).sum()) for c in conf) / points
            ratio_margin = min(ratio_margin, abs(ratio - depth))
            if ratio > depth:
                stop_layer = i
                break
        for s in range(2):
            keep = mt[s] > bar
            if depth > 0:
                keep |= conf[s] <= t[i]
            x[s], enc[s], ind[s] = np.ascontiguousarray(x[s][keep]), np.ascontiguousarray(enc[s][:, keep]), ind[s][keep]
    return len(ind[0]), len(ind[1]), stop_layer, ind[0], ind[1], margin, ratio_margin


def test_the_float64_composition_makes_the_same_decisions():
    """Cases: pruning with and without the conf term at two shapes, and the first of them with depth_confidence 0.567 (stops at layer 1,
    after pruning at layer 0) and 0.45 (stops at layer 0).  In each, no float64 conf or mt lies within PIN of its threshold and no stop
    ratio within 1 / P of depth_confidence, so no rounding of the float32 arithmetic can flip a decision; and the float64 composition
    ends with the restatement's live counts, index maps and stop layer."""
    cases = [(shape, R.prune_case(shape, depth_on)) for shape in (SMALL, SHAPE) for depth_on in (True, False)]
    pruning = R.prune_case(SHAPE, True)
    cases += [(SHAPE, (pruning[0], 0.567, pruning[2])), (SHAPE, (pruning[0], 0.45, pruning[2]))]
    stops = []
    for shape, (case, depth, width) in cases:
        a, b, e0, e1, sd = case
        r = R.run(a, b, shape[3], e0, e1, sd, R.N_LAYERS, depth, width)
        live0, live1, stop_layer, ind0, ind1, margin, ratio_margin = _float64_pass(shape, case, depth, width)
        print(shape[:4], depth, "least distance from a threshold", margin, "of a ratio from depth_confidence", ratio_margin)
        assert margin > PIN and ratio_margin >= 1.0 / (shape[0] + shape[1])
        assert (r.live0, r.live1, r.stop_layer) == (live0, live1, stop_layer)
        assert np.array_equal(r.ind0[:live0], ind0) and np.array_equal(r.ind1[:live1], ind1)
        stops.append(r.stop_layer)
    assert stops == [2, 2, 2, 2, 1, 0]


def _mutant_cases():
    (a, b, e0, e1, sd), depth, width = R.prune_case(SHAPE, True)
    run = lambda sd, depth, width: (lambda v: R.run(a, b, SHAPE[3], e0, e1, sd, R.N_LAYERS, depth, width, variant=v))  # noqa: E731
    yield run(sd, depth, width)   # prunes at both steps, never stops
    # the ratios of that pass: 0.487 after layer 0; after layer 1, 72 unsure of 145 live and P = 195: 0.631, over the live count 0.503
    yield run(sd, 0.567, width)   # prunes at 0, stops at 1
    kwargs, d2, w2 = R.STOP_AT_0
    yield run(R.case(SHAPE, **kwargs)[4], d2, 0.9)  # stops at 0, where the matchability of most rows is below the bar
    # every conf equals t_i to the bit (no token weights, a bias found by search); depth_confidence 1 is never exceeded
    t = R.thresholds(R.N_LAYERS)
    exact = dict(R.split_steer(SHAPE, False), token_scale=0.0, token_bias=(R.bias_hitting(t[0]), R.bias_hitting(t[1])))
    yield run(R.case(SHAPE, **exact)[4], 1.0, width)


def test_the_mutant_cases_are_what_their_comments_say():
    runs = [run(R.CONTRACT) for run in _mutant_cases()]
    assert [(r.stopped, r.stop_layer) for r in runs] == [(0, 2), (1, 1), (1, 0), (0, 2)]
    assert runs[1].live0 + runs[1].live1 == 145 and (runs[3].live0, runs[3].live1) == SHAPE[:2]
    t = R.thresholds(R.N_LAYERS)
    assert (runs[3].conf[0] == t[0]).all() and (runs[3].conf[1] == t[1]).all()


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS), ids=str)
def test_every_mutant_changes_some_output_of_some_case(mutant):
    changed = [not R.same_outputs(run(R.CONTRACT), run(R.MUTANTS[mutant])) for run in _mutant_cases()]
    assert any(changed), mutant


def test_the_restatement_is_the_layers_and_the_head_composed():
    """Without a stop and without pruning: transformer_ref's layers and match_assignment_ref's head, as LightGlue.match composes them."""
    from tests import match_assignment_ref as MA
    from tests import nn_match_ref
    a, b, e0, e1, sd = R.case(SMALL, **R.NEVER[0])
    r = R.run(a, b, SMALL[3], e0, e1, sd, R.N_LAYERS, 0.95, 0.99, count0=20, count1=25)
    x0, x1 = a, b
    for i in range(R.N_LAYERS):
        x0, x1 = T.layer(x0, x1, SMALL[3], e0, e1, sd, f"transformers.{i}.", 20, 25)
    w, bias = R.packed_heads(sd, R.N_LAYERS)
    want = MA.assign(x0, x1, weights=w[2], bias=bias[2], count0=20, count1=25)
    assert T.same(r.scores, want)
    index, status = nn_match_ref.match_scores(want[:33, :31], -1.0e30)
    assert np.array_equal(r.match_index, index) and np.array_equal(r.status, status)
