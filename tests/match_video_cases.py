"""The synthetic sequence the CPU and GPU tests of ``MatchVideoTracker`` share: TEST INFRASTRUCTURE.

40 landmarks, landmark l with descriptor e_l plus seeded noise, renormalised, shown in a permuted order in every frame.  Landmarks 0 .. 4
are hidden for two frames (2, 3), landmarks 5 .. 9 for three (2, 3, 4); 40 .. 43 appear in frame 3 and 44, 45 in frame 6.  With
``max_lost = 2`` the first group keeps its ids and the second returns under new ones.  ``expected_ids`` is that history written down from
the rules alone (admission is in ascending current row, ids count up from 0); ``compose`` is the same sequence through the restatements
(match_assignment_ref.c, nn_match_ref.c, match_table_ref).

Why the numbers separate: a true pair's cosine is about 0.97 and a false pair's within +-0.1, so with ``SCALE`` squared = 20.25 a true
pair's two softmaxes are within e^-17 of 1 (score about 0) and every other entry of its row and column is below -17; a hidden landmark's
row has no such column, its best entry loses the column's softmax to that column's true row, and a new keypoint's column likewise.
``MIN_SCORE`` -3 lies between the two by more than five units either way.
"""
import functools

import numpy as np

from tests import match_assignment_ref as MA
from tests import match_table_ref as R
from tests import nn_match_ref as NM

DIM, SLOTS, FRAMES, MAX_LOST = 64, 64, 8, 2
SCALE, NOISE, MIN_SCORE = 4.5, 0.02, -3.0
SHORT, LONG = range(0, 5), range(5, 10)   # hidden in frames 2, 3 / in frames 2, 3, 4
LATE = {3: range(40, 44), 6: range(44, 46)}  # the frame in which new landmarks appear
IMAGE = (128, 96)  # (W, H)


def visible(frame):
    """The landmarks frame ``frame`` shows, ascending."""
    seen = []
    for l in range(46):
        if l in SHORT and frame in (2, 3):
            continue
        if l in LONG and frame in (2, 3, 4):
            continue
        if l >= 40 and not any(l in late and frame >= first for first, late in LATE.items()):
            continue
        seen.append(l)
    return seen


@functools.lru_cache(maxsize=None)
def frame(f, seed=7):
    """(landmark of every current row, uv [K, 2], descriptors [K, DIM]) of frame ``f``, read-only."""
    rng = np.random.default_rng(1000 * seed + f)
    order = np.array(visible(f))[rng.permutation(len(visible(f)))]
    desc = np.eye(46, DIM)[order] + NOISE * rng.standard_normal((len(order), DIM))
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(np.float32)
    # a landmark drifts by (1.5, 0.5) pixels per frame from its own place on a grid
    uv = np.stack([10.0 + 14.0 * (order % 8) + 1.5 * f, 8.0 + 13.0 * (order // 8) + 0.5 * f], 1).astype(np.float32)
    for a in (order, uv, desc):
        a.setflags(write=False)
    return order, uv, desc


def expected_ids():
    """Per frame {landmark: id} of the live tracks, from the rules alone."""
    history, ids, next_id, last_seen = [], {}, 0, {}
    for f in range(FRAMES):
        order = frame(f)[0]
        for l in order:  # ascending current row: a landmark without a live track gets the next id
            if l not in ids:
                ids[l] = next_id
                next_id += 1
            last_seen[l] = f
        for l in [l for l in ids if f - last_seen[l] > MAX_LOST]:  # a track dies in the frame of its (MAX_LOST + 1)-th miss in a row
            del ids[l]
        history.append(dict(ids))
    return history


def compose(frames=FRAMES, mutant=None):
    """The sequence through the restatements: per frame (the table after it as a dict of copies, cur_slot)."""
    table, out = R.Table(SLOTS, DIM), []
    for f in range(frames):
        _, uv, desc = frame(f)
        q_uv, q_desc, q_slot, q_count = table.query()
        if f == 0:
            index, status = np.full(SLOTS, -1, np.int32), np.full(SLOTS, R.LARGE_RESIDUAL, np.uint8)
        else:
            scores = MA.assign(q_desc, desc, scale=SCALE, count0=int(q_count[0]))
            index, status = NM.match_scores(scores[:SLOTS, :len(uv)], MIN_SCORE)
        cur_slot = table.update(q_slot, q_count[0], index, status, uv, desc, None, MAX_LOST, mutant=mutant)
        out.append(({k: v.copy() for k, v in table.tensors().items()}, cur_slot))
    return out


def ids_by_landmark(f, tensors, cur_slot):
    """{landmark: id} of the landmarks frame ``f`` shows, through cur_slot."""
    order = frame(f)[0]
    return {int(l): int(tensors["ids"][cur_slot[j]]) if cur_slot[j] >= 0 else None for j, l in enumerate(order)}
