"""Per-frame time of MatchVideoTracker against the per-pair composition with the id bookkeeping on the host.

A translated synthetic sequence with seeded random upstream-width weights (SuperPoint 64-64-128-128-256-256, LightGlue D = 256, 4 heads,
9 layers) at 752 x 480 with 300 keypoints and tracks and at 640 x 480 with 1 024.  Three rows per shape, each the median and p10 - p90 of
the timed frames, every frame bracketed by a device synchronisation:
  (i)   tracker      a ``MatchVideoTracker.track`` frame;
  (ii)  composition  the README's per-pair snippet as a caller had to write it: ``detect`` on both images, ``match``, ``match_index.cpu()``
                     and a dict from keypoint row to id;
  (iii) table        the query and update launches alone, on the tracker's own tensors.
Random weights give arbitrary matches: the rows compare the cost of the two loops, not the quality of their tracks.  One JSON line per
shape (appended to --out when given)."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_scenes import HEADS, WIDTHS, make_state, sequence, state_dict  # noqa: E402
from scripts.benchlib import parser, percentiles, wall_time, write_rows  # noqa: E402

SHAPES = {"euroc_752x480": (752, 480, 300), "vga_640x480": (640, 480, 1024)}


def timed_frames(torch, images, frame):
    return [wall_time(torch, lambda: frame(k, image)) for k, image in enumerate(images)]


def composition(F, sp, decoder, lg, size, images):
    """The loop a caller had to write: the detector runs on both images of every pair, and the ids live in a Python dict."""
    ids, next_id = {}, [0]

    def frame(k, image):
        cur = sp.detect(image, decoder)
        if k == 0:
            for j in range(int(cur.count.item())):
                ids[j] = next_id[0]
                next_id[0] += 1
            return
        prev = sp.detect(images[k - 1], decoder)
        # (detect reuses the network's buffers per image size, the decoder's outputs are the call's own)
        _, match_index, _ = lg.match(prev.uv, cur.uv, prev.descriptors, cur.descriptors, size, size, prev.count, cur.count)
        index = match_index.cpu().numpy()  # the read-back
        moved, taken = {}, set()
        for i, j in enumerate(index.tolist()):
            if j >= 0 and i in ids:
                moved[j] = ids[i]
                taken.add(j)
        for j in range(int(cur.count.item())):
            if j not in taken:
                moved[j] = next_id[0]
                next_id[0] += 1
        ids.clear()
        ids.update(moved)

    return frame, ids


def spread(times, warmup):
    return dict(zip(("median", "p10", "p90"), (round(v, 1) for v in percentiles(1e6 * np.asarray(times[warmup:])))))


def rows(args, torch):
    import feature_tracker_amd as F
    from feature_tracker_amd._device_match_table import match_table_query_args, match_table_update_args
    from feature_tracker_amd._torch_call import call, context_of

    sp = F.SuperPoint.from_state_dict(make_state(torch, WIDTHS, 1))
    sd = state_dict(torch, np.random.default_rng(1))
    for name, (width, height, n) in SHAPES.items():
        images = [torch.from_numpy(i.astype(np.float32) / np.float32(255.0)).cuda() for i in sequence(width, height, args.frames + args.warmup)]
        decoder = F.KeypointDecoder(max_keypoints=n, min_score=0.0, min_distance=4, border=4)  # seeded weights: every score is near 1 / 65
        tracker = F.MatchVideoTracker(F.LightGlue.from_state_dict(sd, num_heads=HEADS), n, max_lost=2, detector=(sp, decoder))
        t_tracker = timed_frames(torch, images, lambda k, image: tracker.track(image))
        frame, ids = composition(F, sp, decoder, F.LightGlue.from_state_dict(sd, num_heads=HEADS), (width, height), images)
        t_composition = timed_frames(torch, images, frame)
        # (iii): the four launches on the tracker's tensors, with the last frame's matches
        t, ctx = tracker, context_of(tracker.ids)
        found = sp.detect(images[-1], decoder)
        index = torch.randint(-1, n, (n,), dtype=torch.int32, device="cuda")
        status = torch.randint(1, 3, (n,), dtype=torch.uint8, device="cuda")
        per = t._per_rows[n]

        def table(k, image):
            call("ftk_match_table_query_device", match_table_query_args(ctx, t.ids, t.points, t.descriptors, t._q_uv, t._q_desc, t._q_slot, t._q_count), ctx)
            call("ftk_match_table_update_device", match_table_update_args(
                ctx, t.ids, t.points, t.prev_points, t.descriptors, t.status, t.age, t.lost, t.n_live, t.next_id, t._q_slot, t._q_count, index, status,
                found.uv, found.descriptors, found.count, t.max_lost, per["workspace"], per["cur_slot"]), ctx)

        t_table = timed_frames(torch, images, table)
        row = {"bench": "match_video", "shape": name, "width": width, "height": height, "max_tracks": n, "frames": args.frames,
               "tracker_us": spread(t_tracker, args.warmup), "composition_us": spread(t_composition, args.warmup), "table_us": spread(t_table, args.warmup),
               "tracker_live": int(tracker.n_live.item()), "composition_live": len(ids), "device": torch.cuda.get_device_name(0)}
        row["speedup"] = round(row["composition_us"]["median"] / row["tracker_us"]["median"], 2)
        yield row


def main():
    args = parser("--frames", 30, 5, os.path.join(ROOT, "profiles", "match_video_bench.jsonl")).parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=True)


if __name__ == "__main__":
    main()
