"""The inputs more than one bench script uses, each defined once: the camera, the synthetic scenes and sequences, the seeded weights and the
shape tables.  Seeds and draw order are part of the published figures' conditions (tests/test_benchlib_cpu.py pins the arrays)."""
from __future__ import annotations

import numpy as np

K = (512.0, 512.0, 319.5, 239.5)  # fx, fy, cx, cy: the camera of both scenes below
IMAGE = (480, 640)

# bench_klt_video.py and the trackers with a filter: width, height, features, minimum distance
VIDEO_SHAPES = {"reference": (752, 480, 300, 25), "headline": (640, 480, 2000, 8)}
# bench_raft.py: (name, (hidden, feature, context, levels, radius, corr_hidden, corr_out, flow_hidden, flow_out, motion_out, mask_hidden), B, H, W, iterations)
RAFT_SHAPES = [("model_py_60x60", (64, 128, 128, 3, 3, 64, 32, 32, 16, 32, 64), 5, 60, 60, 5),
               ("raft_440x1024", (128, 256, 128, 4, 4, 256, 192, 128, 64, 128, 256), 1, 440, 1024, 12)]
# bench_raft_corr.py: (name, C, H, W, levels, radius)
CORR_SHAPES = [("eighth_example_c128", 128, 60, 94, 3, 3), ("eighth_example_c256", 256, 60, 94, 4, 4), ("raft_55x128_c256", 256, 55, 128, 4, 4)]
# LightGlue as bench_transformer_layer.py times it
SIZES = (300, 1024, 2048)
DIM, HEADS, LAYERS = 256, 4, 9
# SuperPoint's upstream widths: conv1, conv2, conv3, conv4, the heads' hidden layers, D
WIDTHS = (64, 64, 128, 128, 256, 256)


def two_view_scene(n, seed=1):
    """Correspondences of a translating, slightly rotating camera over random depths, 30 % of them replaced by random points."""
    rng = np.random.default_rng(seed)
    H, W = IMAGE
    f = 0.8 * W
    ref = rng.uniform([10, 10], [W - 10, H - 10], (n, 2))
    depth = rng.uniform(2.0, 10.0, n)
    X = np.c_[(ref[:, 0] - 0.5 * (W - 1)) / f, (ref[:, 1] - 0.5 * (H - 1)) / f, np.ones(n)] * depth[:, None]
    a = 0.03
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Y = X @ R.T + np.array([0.5, 0.1, 0.15])
    cur = np.c_[f * Y[:, 0] / Y[:, 2] + 0.5 * (W - 1), f * Y[:, 1] / Y[:, 2] + 0.5 * (H - 1)]
    out = rng.permutation(n)[:int(0.3 * n)]
    cur[out] = rng.uniform([5, 5], [W - 5, H - 5], (len(out), 2))
    return ref.astype(np.float32), cur.astype(np.float32)


def landmark_scene(n, seed=1, outlier_share=0.3, noise=0.3):
    """n landmarks 4.5 to 7.5 deep seen by a camera a small motion away, 0.3 px noise, 30 % of the pixels redrawn: (landmarks, uv)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    a = np.array([0.03, -0.05, 0.02])
    Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
    Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
    R, t = Rz @ Ry @ Rx, np.array([0.5, 0.1, 0.15])
    X = np.array([0.0, 0.0, 6.0]) + rng.uniform(-1.5, 1.5, (n, 3))
    Y = X @ R.T + t
    uv = np.c_[fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy] + rng.normal(0.0, noise, (n, 2))
    out = rng.permutation(n)[:int(round(n * outlier_share))]
    uv[out] = rng.uniform([5, 5], [IMAGE[1] - 5, IMAGE[0] - 5], (len(out), 2))
    return X.astype(np.float32), uv.astype(np.float32)


def sequence(width, height, frames):
    from feature_tracker_amd import synth
    big = synth.make_image_pair(width + 2 * frames, height + frames, (0.0, 0.0))[0]
    return [np.ascontiguousarray(big[k:k + height, 2 * k:2 * k + width]) for k in range(frames)]  # the camera moves by (2, 1) pixels a frame


def state_dict(torch, rng):
    sd, d = {}, DIM
    lin = lambda outs, ins: (torch.from_numpy((rng.standard_normal((outs, ins)) / np.sqrt(ins)).astype(np.float32)).cuda(),  # noqa: E731
                             torch.from_numpy((0.1 * rng.standard_normal(outs)).astype(np.float32)).cuda())
    for i in range(LAYERS):
        for block, names in (("self_attn", (("Wqkv", 3 * d, d), ("out_proj", d, d))), ("cross_attn", (("to_qk", d, d), ("to_v", d, d), ("to_out", d, d)))):
            for name, outs, ins in names + (("ffn.0", 2 * d, 2 * d), ("ffn.3", d, 2 * d)):
                sd[f"transformers.{i}.{block}.{name}.weight"], sd[f"transformers.{i}.{block}.{name}.bias"] = lin(outs, ins)
            sd[f"transformers.{i}.{block}.ffn.1.weight"], sd[f"transformers.{i}.{block}.ffn.1.bias"] = torch.ones(2 * d).cuda(), torch.zeros(2 * d).cuda()
    sd["posenc.Wr.weight"] = torch.from_numpy(rng.standard_normal((d // HEADS // 2, 2)).astype(np.float32)).cuda()
    head = f"log_assignment.{LAYERS - 1}."
    sd[head + "final_proj.weight"], sd[head + "final_proj.bias"] = lin(d, d)
    sd[head + "matchability.weight"], sd[head + "matchability.bias"] = lin(1, d)
    return sd


def lightglue_inputs(torch, rng, n, size):
    """n unit descriptors, a permuted and perturbed copy of them, and keypoints for both on an image of ``size``: (a, b, kp0, kp1)."""
    x = rng.standard_normal((n, DIM))
    y = x[rng.permutation(n)] + 0.3 * rng.standard_normal((n, DIM))
    a = torch.from_numpy((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)).cuda()
    b = torch.from_numpy((y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)).cuda()
    kp0 = torch.from_numpy((rng.random((n, 2)) * np.array(size)).astype(np.float32)).cuda()
    kp1 = torch.from_numpy((rng.random((n, 2)) * np.array(size)).astype(np.float32)).cuda()
    return a, b, kp0, kp1


def make_state(torch, widths, seed):
    c1, c2, c3, c4, head, d = widths
    shapes = {"conv1a": (c1, 1, 3), "conv1b": (c1, c1, 3), "conv2a": (c2, c1, 3), "conv2b": (c2, c2, 3), "conv3a": (c3, c2, 3), "conv3b": (c3, c3, 3),
              "conv4a": (c4, c3, 3), "conv4b": (c4, c4, 3), "convPa": (head, c4, 3), "convPb": (65, head, 1), "convDa": (head, c4, 3), "convDb": (d, head, 1)}
    torch.manual_seed(seed)
    state = {}
    for name, (M, Cin, ks) in shapes.items():
        conv = torch.nn.Conv2d(Cin, M, ks, stride=1, padding=ks // 2)
        state[name + ".weight"], state[name + ".bias"] = conv.weight.detach().cuda(), conv.bias.detach().cuda()
    return state
