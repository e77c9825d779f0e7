"""``attention``, ``TransformerLayer`` and ``LightGlue``: LightGlue's self- and cross-attention on the device.

A layer is the self block on each descriptor set (a Linear to q, k and v, the rotary encoding, softmax attention, a Linear, and a
two-layer FFN with LayerNorm and GELU on ``[x | message]``) and then the cross block in both directions.  12 launches on one stream, on
tensors that stay where they are: no copy to the host, no count read back, no synchronisation.  ``LightGlue`` composes the optional
input projection, the rotary encoding (torch ops, once per image), the layers and ``MatchAssignment``.
"""
from __future__ import annotations

import math

from . import _native as N
from ._device_lightglue_adaptive import (check_confidence, check_min_keypoints, lightglue_adapt_step_args, lightglue_confidence_args,
                                         lightglue_finish_args, stop_threshold, transformer_layer_adaptive_args)
from ._device_transformer import attention_args, check_heads, check_rows, linear_args, transformer_layer_args
from ._torch_call import OnStream, PerKey, call, check_ctx, complain, words

_SELF = ("self_attn.Wqkv", "self_attn.out_proj", "self_attn.ffn.0", "self_attn.ffn.1", "self_attn.ffn.3")
_CROSS = ("cross_attn.to_qk", "cross_attn.to_v", "cross_attn.to_out", "cross_attn.ffn.0", "cross_attn.ffn.1", "cross_attn.ffn.3")


def attention(q, k, v, count=None, pre_scale=1.0, post_scale=None, ctx=None):
    """``softmax((q pre_scale)(k pre_scale)^T post_scale) v`` per head, in DESIGN.md 5.24's arithmetic.  ``q``: float32 CUDA [M, h, dh],
    ``k`` and ``v``: [N, h, dh], contiguous (views of [rows, h * dh]); ``count``: an optional int32 [1] device tensor, only the first
    ``clamp(count, 0, N)`` keys are valid; ``post_scale`` None: ``dh ** -0.5``.  Returns [M, h, dh]; no valid key gives zeros.  One
    launch, nothing read back."""
    from . import device as D

    check_ctx(ctx)
    tensors = [("q", q, D._F32, (None, None, None))]
    complain(tensors[:1], cuda=False)
    m, h, dh = (int(e) for e in q.shape)
    tensors += [("k", k, D._F32, (None, h, dh))]
    complain(tensors[1:], cuda=False)
    tensors += [("v", v, D._F32, (int(k.shape[0]), h, dh))]
    if count is not None:
        tensors.append(("count", count, D._I32, (1,)))
    complain(tensors)
    with OnStream(ctx, q) as on:
        out = on.torch.empty_like(q)
        call("ftk_attention_device", attention_args(on.ctx, q, k, v, count, pre_scale, post_scale, out, on.stream), on.ctx)
    return out


def _linear_pair(sd, name):
    import torch

    out = []
    for part in ("weight", "bias"):
        key = f"{name}.{part}"
        if key not in sd:
            raise ValueError(f"the state dict lacks {key!r}")
        t = sd[key]
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{key} must be a float32 tensor (got {getattr(t, 'dtype', type(t).__name__)})")
        out.append(t.detach())
    return out


def _shaped(key, t, shape):
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{key} must be {list(shape)} (got {list(t.shape)})")
    return t


def _check_size(name, size):
    """An image size as ``rotary_encoding`` takes it: (width, height), two finite numbers > 0."""
    try:
        w, h = (float(e) for e in size)
    except (TypeError, ValueError):
        w = h = math.nan
    if not (math.isfinite(w) and math.isfinite(h) and w > 0 and h > 0):
        raise ValueError(f"{name} must be (width, height), two finite numbers > 0 (got {size!r})")


def rotary_encoding(kpts, size, Wr):
    """Upstream's positional encoding in torch ops: ``normalize_keypoints`` (``(kpts - size / 2) / (max(size) / 2)``), ``Wr`` [dh / 2, 2],
    ``cos`` / ``sin``, ``repeat_interleave(2)``: float32 [2, rows, dh].  ``kpts``: [rows, 2] pixels; ``size``: (width, height).  An input
    to DESIGN.md 5.24's contract, not part of it: computed once per image and reused by every layer."""
    import torch

    size = torch.as_tensor(size, dtype=kpts.dtype, device=kpts.device)
    normalised = (kpts - size / 2) / (size.max() / 2)
    projected = normalised @ Wr.to(kpts.device).t()
    return torch.stack([torch.cos(projected), torch.sin(projected)], 0).repeat_interleave(2, dim=-1).contiguous()


class TransformerLayer:
    """``TransformerLayer.from_state_dict(sd, "transformers.0.")``, then ``layer(desc0, desc1, enc0, enc1)``.

    ``desc0``: float32 CUDA [M, D], ``desc1``: [N, D], contiguous; ``enc0`` [2, M, dh], ``enc1`` [2, N, dh]: ``rotary_encoding``'s cos and
    sin.  ``count0`` / ``count1``: optional int32 [1] device tensors (``KeypointDecoder``'s ``count``): rows at or behind
    ``clamp(count, 0, rows)`` take part in no softmax as keys; as queries they are computed like any other row and hold finite garbage
    that ``MatchAssignment``'s counts discard.  Returns ``(desc0', desc1')`` as new tensors.  The bits are those of DESIGN.md 5.24's
    contract, which the tests hold to a scalar restatement.

    Limits: 1 <= M, N <= 4 096, D <= 1 024, ``num_heads`` divides D, the head dimension even and in 2 .. 128; float32, one pair per
    call, inference only.  The kernels run on torch's current stream (or on ``ctx``'s, from ``device.context_on_stream``); the object
    keeps one workspace per (device, M, N), so a call captured after one eager call at that size allocates nothing but its outputs.
    There is no CPU fallback."""

    def __init__(self, dim: int, num_heads: int, packed, ctx=None):
        self.head_dim = check_heads(dim, num_heads)
        check_ctx(ctx)
        self.dim, self.num_heads = dim, num_heads
        self._packed = {packed.device: packed}
        self._ctx = ctx
        self._workspace = PerKey()  # (device, M, N) -> the workspace of that size

    @classmethod
    def from_state_dict(cls, sd, prefix: str = "transformers.0.", num_heads: int = 4, ctx=None) -> "TransformerLayer":
        """Upstream LightGlue's tensors ``{prefix}self_attn.{Wqkv, out_proj, ffn.0, ffn.1, ffn.3}`` and ``{prefix}cross_attn.{to_qk, to_v,
        to_out, ffn.0, ffn.1, ffn.3}`` (``weight`` and ``bias`` each), packed once into one flat tensor.  ``Wqkv``'s rows, which upstream
        reads as (head, channel, q | k | v), are regrouped into q, k and v planes.  ``D`` is read off the weights."""
        import torch

        tensors = {name: _linear_pair(sd, prefix + name) for name in _SELF + _CROSS}
        wqkv = tensors["self_attn.Wqkv"][0]
        if wqkv.dim() != 2 or wqkv.shape[0] != 3 * wqkv.shape[1]:
            raise ValueError(f"{prefix}self_attn.Wqkv.weight must be [3 D, D] (got {list(wqkv.shape)})")
        d = int(wqkv.shape[1])
        check_heads(d, num_heads)
        shapes = {"self_attn.Wqkv": (3 * d, d), "self_attn.out_proj": (d, d), "cross_attn.to_qk": (d, d), "cross_attn.to_v": (d, d), "cross_attn.to_out": (d, d)}
        for block in ("self_attn", "cross_attn"):
            shapes.update({f"{block}.ffn.0": (2 * d, 2 * d), f"{block}.ffn.1": (2 * d,), f"{block}.ffn.3": (d, 2 * d)})
        for name, (w, b) in tensors.items():
            _shaped(f"{prefix}{name}.weight", w, shapes[name])
            _shaped(f"{prefix}{name}.bias", b, shapes[name][:1])
        device = wqkv.device
        get = lambda name: [t.to(device) for t in tensors[name]]  # noqa: E731
        wq, bq = get("self_attn.Wqkv")
        planes = [wq.view(d, 3, d).permute(1, 0, 2).reshape(3 * d, d), bq.view(d, 3).t().reshape(3 * d)]
        (wk, bk), (wv, bv) = get("cross_attn.to_qk"), get("cross_attn.to_v")
        parts = planes + get("self_attn.out_proj") + get("self_attn.ffn.0") + get("self_attn.ffn.1") + get("self_attn.ffn.3")
        parts += [torch.cat([wk, wv], 0), torch.cat([bk, bv], 0)] + get("cross_attn.to_out") + get("cross_attn.ffn.0") + get("cross_attn.ffn.1")
        parts += get("cross_attn.ffn.3")
        packed = torch.cat([t.reshape(-1) for t in parts]).contiguous()
        assert packed.numel() == N.transformer_layer_weight_offsets(d)[2]
        return cls(d, num_heads, packed, ctx)

    def _validate(self, desc0, desc1, enc0, enc1, count0, count1):
        from . import device as D

        tensors = [("desc0", desc0, D._F32, (None, self.dim)), ("desc1", desc1, D._F32, (None, self.dim))]
        complain(tensors, cuda=False)
        m, n = int(desc0.shape[0]), int(desc1.shape[0])
        check_rows("desc0 and desc1", m, n)
        tensors += [("enc0", enc0, D._F32, (2, m, self.head_dim)), ("enc1", enc1, D._F32, (2, n, self.head_dim))]
        if count0 is not None:
            tensors.append(("count0", count0, D._I32, (1,)))
        if count1 is not None:
            tensors.append(("count1", count1, D._I32, (1,)))
        complain(tensors)
        return m, n

    def __call__(self, desc0, desc1, enc0, enc1, count0=None, count1=None):
        m, n = self._validate(desc0, desc1, enc0, enc1, count0, count1)
        with OnStream(self._ctx, desc0) as on:
            out = self._run(on, desc0, desc1, enc0, enc1, count0, count1, m, n)
        return out

    def _run(self, on, desc0, desc1, enc0, enc1, count0, count1, m, n):
        torch, device = on.torch, desc0.device
        if device not in self._packed:
            self._packed[device] = next(iter(self._packed.values())).to(device)
        workspace = self._workspace.of((device, m, n), lambda: words(torch, N.transformer_layer_workspace_bytes(m, n, self.dim, self.num_heads), device))
        out0, out1 = torch.empty_like(desc0), torch.empty_like(desc1)
        call("ftk_transformer_layer_device", transformer_layer_args(on.ctx, desc0, desc1, self.num_heads, enc0, enc1, self._packed[device], count0, count1,
                                                                    workspace, out0, out1, on.stream), on.ctx)
        return out0, out1


class LightGlue:
    """``LightGlue.from_state_dict(sd)``, then ``scores(...)`` or ``match(...)``: upstream LightGlue's forward pass from keypoints and
    descriptors to the log-assignment tensor, as a composition of the optional ``input_proj`` (linear_kernel), ``rotary_encoding``,
    ``n_layers`` ``TransformerLayer`` s and ``MatchAssignment`` of the last layer.

    ``kpts0`` [M, 2], ``kpts1`` [N, 2]: float32 CUDA pixel coordinates; ``desc0`` [M, D_in], ``desc1`` [N, D_in]; ``size0`` / ``size1``:
    (width, height) of the images; ``count0`` / ``count1``: optional int32 [1] device tensors.  Everything runs on one stream and nothing
    is read on the host; the layers share one workspace per (device, M, N).  ``match_adaptive`` is upstream's forward pass with
    ``depth_confidence`` (early stopping) and ``width_confidence`` (point pruning), DESIGN.md 5.26.  Out of scope: a host-synchronising
    mode that skips the launches of a stopped layer, a batch dimension, a C++ class."""

    def __init__(self, layers, head, Wr, input_proj=None, ctx=None, adaptive=None):
        check_ctx(ctx)
        self.layers, self.head, self.Wr, self.input_proj, self._ctx = list(layers), head, Wr, input_proj, ctx
        # (depth_confidence, width_confidence, pruning_min_keypoints, token_w [L, D], token_b [L], head_w [L, D + 1, D], head_b [L, D + 1])
        self._adaptive = adaptive
        self._adaptive_moved = {}
        self._adaptive_buffers = PerKey()  # (device, M, N) -> the pass's buffers
        self._adaptive_sizes = {}    # (device, width, height) -> the image size on the device
        self.dim, self.num_heads = self.layers[0].dim, self.layers[0].num_heads
        self._moved = {}
        # the layers run one after another on one stream: one workspace per (device, M, N) serves them all
        self._workspace = PerKey()
        for layer in self.layers:
            layer._workspace = self._workspace

    @classmethod
    def from_state_dict(cls, sd, num_heads: int = 4, n_layers=None, ctx=None, depth_confidence=-1, width_confidence=-1,
                        pruning_min_keypoints: int = 1024) -> "LightGlue":
        """Upstream's state dict: ``posenc.Wr.weight``, ``transformers.{i}.*``, ``log_assignment.{n_layers - 1}.*`` and, where the input
        dimension differs, ``input_proj.{weight, bias}``.  ``n_layers`` None: every layer the state dict holds.  With
        ``depth_confidence`` or ``width_confidence`` > 0 (upstream: 0.95 and 0.99; ``pruning_min_keypoints``: upstream's CUDA default)
        also ``token_confidence.{i}.token.0.{weight, bias}`` and ``log_assignment.{i}.*`` of every layer, for ``match_adaptive``."""
        import torch

        from .match_assignment import MatchAssignment

        depth = check_confidence("depth_confidence", depth_confidence)
        width = check_confidence("width_confidence", width_confidence)
        check_min_keypoints(pruning_min_keypoints)

        if n_layers is None:
            n_layers = 0
            while f"transformers.{n_layers}.self_attn.Wqkv.weight" in sd:
                n_layers += 1
        if isinstance(n_layers, bool) or not isinstance(n_layers, int) or n_layers < 1:
            raise ValueError(f"n_layers must be a positive integer and the state dict must hold transformers.0 (got {n_layers!r})")
        layers = [TransformerLayer.from_state_dict(sd, f"transformers.{i}.", num_heads, ctx) for i in range(n_layers)]
        head = MatchAssignment.from_state_dict(sd, f"log_assignment.{n_layers - 1}.", ctx)
        if head.dim != layers[0].dim or any(layer.dim != layers[0].dim for layer in layers):
            raise ValueError("the layers and the assignment head must share one D")
        if "posenc.Wr.weight" not in sd:
            raise ValueError("the state dict lacks 'posenc.Wr.weight'")
        Wr = sd["posenc.Wr.weight"]
        if not isinstance(Wr, torch.Tensor) or Wr.dtype != torch.float32 or tuple(Wr.shape) != (layers[0].head_dim // 2, 2):
            raise ValueError(f"posenc.Wr.weight must be a float32 tensor of shape [{layers[0].head_dim // 2}, 2] (got "
                             f"{getattr(Wr, 'dtype', type(Wr).__name__)} {list(getattr(Wr, 'shape', []))})")
        input_proj = None
        if "input_proj.weight" in sd:
            w, b = _linear_pair(sd, "input_proj")
            if w.dim() != 2 or w.shape[0] != layers[0].dim or not 1 <= w.shape[1] <= N.FTK_TRANSFORMER_MAX_DIM:
                raise ValueError(f"input_proj.weight must be [{layers[0].dim}, 1 .. {N.FTK_TRANSFORMER_MAX_DIM}] (got {list(w.shape)})")
            _shaped("input_proj.bias", b, (layers[0].dim,))
            input_proj = (w.contiguous(), b.contiguous())
        adaptive = None
        if depth > 0 or width > 0:
            if n_layers > N.FTK_LIGHTGLUE_MAX_LAYERS:
                raise ValueError(f"the adaptive pass takes at most FTK_LIGHTGLUE_MAX_LAYERS = {N.FTK_LIGHTGLUE_MAX_LAYERS} layers (got {n_layers})")
            d = layers[0].dim
            wanted = [f"token_confidence.{i}.token.0.{part}" for i in range(n_layers - 1) for part in ("weight", "bias")]
            wanted += [f"log_assignment.{i}.{k}" for i in range(n_layers) for k in ("final_proj.weight", "final_proj.bias", "matchability.weight",
                                                                                     "matchability.bias")]
            missing = [k for k in wanted if k not in sd]
            if missing:
                raise ValueError(f"depth_confidence / width_confidence need tensors the state dict lacks: {missing}")
            device = head._packed[next(iter(head._packed))][0].device
            token_w, token_b = torch.zeros((n_layers, d), dtype=torch.float32, device=device), torch.zeros((n_layers,), dtype=torch.float32, device=device)
            for i in range(n_layers - 1):
                w, b = _linear_pair(sd, f"token_confidence.{i}.token.0")
                token_w[i] = _shaped(f"token_confidence.{i}.token.0.weight", w, (1, d)).to(device)[0]
                token_b[i] = _shaped(f"token_confidence.{i}.token.0.bias", b, (1,)).to(device)[0]
            heads = [MatchAssignment.from_state_dict(sd, f"log_assignment.{i}.", ctx) for i in range(n_layers)]
            if any(h.dim != d for h in heads):
                raise ValueError("the layers and every assignment head must share one D")
            head_w = torch.stack([next(iter(h._packed.values()))[0].to(device) for h in heads]).contiguous()
            head_b = torch.stack([next(iter(h._packed.values()))[1].to(device) for h in heads]).contiguous()
            adaptive = (depth, width, pruning_min_keypoints, token_w, token_b, head_w, head_b)
        return cls(layers, head, Wr.detach(), input_proj, ctx, adaptive)

    def _validate(self, kpts0, kpts1, desc0, desc1, size0, size1, count0, count1, min_score=None):
        from . import device as D

        for name, size in (("size0", size0), ("size1", size1)):
            _check_size(name, size)
        if min_score is not None and (isinstance(min_score, bool) or not isinstance(min_score, (int, float)) or math.isnan(min_score)):
            raise ValueError(f"min_score must be a number (got {min_score!r})")
        d_in = self.dim if self.input_proj is None else int(self.input_proj[0].shape[1])
        tensors = [("desc0", desc0, D._F32, (None, d_in)), ("desc1", desc1, D._F32, (None, d_in))]
        complain(tensors, cuda=False)
        m, n = int(desc0.shape[0]), int(desc1.shape[0])
        check_rows("desc0 and desc1", m, n)
        tensors += [("kpts0", kpts0, D._F32, (m, 2)), ("kpts1", kpts1, D._F32, (n, 2))]
        if count0 is not None:
            tensors.append(("count0", count0, D._I32, (1,)))
        if count1 is not None:
            tensors.append(("count1", count1, D._I32, (1,)))
        complain(tensors)
        return m, n

    def _inputs(self, on, kpts0, kpts1, desc0, desc1, size0, size1):
        """The projected descriptors and the rotary encodings: what the first layer reads."""
        torch, device = on.torch, desc0.device
        if device not in self._moved:
            proj = None if self.input_proj is None else tuple(t.to(device) for t in self.input_proj)
            self._moved[device] = (self.Wr.to(device), proj)
        Wr, proj = self._moved[device]
        if proj is not None:
            projected = []
            for x in (desc0, desc1):
                out = torch.empty((int(x.shape[0]), self.dim), dtype=torch.float32, device=device)
                call("ftk_linear_device", linear_args(on.ctx, x, proj[0], proj[1], out, on.stream), on.ctx)
                projected.append(out)
            desc0, desc1 = projected
        return desc0, desc1, rotary_encoding(kpts0, size0, Wr), rotary_encoding(kpts1, size1, Wr)

    def _descriptors(self, on, kpts0, kpts1, desc0, desc1, size0, size1, count0, count1, m, n):
        desc0, desc1, enc0, enc1 = self._inputs(on, kpts0, kpts1, desc0, desc1, size0, size1)
        for layer in self.layers:
            desc0, desc1 = layer._run(on, desc0, desc1, enc0, enc1, count0, count1, m, n)
        return desc0, desc1

    def scores(self, kpts0, kpts1, desc0, desc1, size0, size1, count0=None, count1=None):
        """``scores`` float32 [M + 1, N + 1], as ``MatchAssignment.assign`` lays it out."""
        m, n = self._validate(kpts0, kpts1, desc0, desc1, size0, size1, count0, count1)
        with OnStream(self._ctx, desc0) as on:
            desc0, desc1 = self._descriptors(on, kpts0, kpts1, desc0, desc1, size0, size1, count0, count1, m, n)
            result = self.head.assign(desc0, desc1, count0, count1)
        return result

    def match(self, kpts0, kpts1, desc0, desc1, size0, size1, count0=None, count1=None, min_score: float = -1.0e30):
        """``(scores, match_index int32 [M], status uint8 [M])``, as ``MatchAssignment.match`` returns them."""
        m, n = self._validate(kpts0, kpts1, desc0, desc1, size0, size1, count0, count1, min_score)
        with OnStream(self._ctx, desc0) as on:
            desc0, desc1 = self._descriptors(on, kpts0, kpts1, desc0, desc1, size0, size1, count0, count1, m, n)
            result = self.head.match(desc0, desc1, count0, count1, min_score=min_score)
        return result

    # ---- the adaptive pass ----

    def _adaptive_state(self, on, device, m, n):
        """The packed heads on ``device`` and the pass's buffers of this size, made on the first call."""
        torch = on.torch
        if device not in self._adaptive_moved:
            self._adaptive_moved[device] = tuple(t.to(device) for t in self._adaptive[3:])
        return self._adaptive_moved[device], self._adaptive_buffers.of((device, m, n), lambda: self._adaptive_allocate(torch, device, m, n))

    def _adaptive_allocate(self, torch, device, m, n):
        dh, L = self.layers[0].head_dim, len(self.layers)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)  # noqa: E731
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=device)  # noqa: E731
        return dict(halves=[(f32(m, self.dim), f32(n, self.dim), f32(2, m, dh), f32(2, n, dh), i32(m), i32(n)) for _ in range(2)],
                    conf=f32(m + n), mt=f32(m + n), scores=f32(m + 1, n + 1), match_index=i32(m),
                    status=torch.empty((m,), dtype=torch.uint8, device=device), state=i32(N.FTK_LIGHTGLUE_STATE_WORDS), layers=i32(m + n),
                    identity=torch.arange(max(m, n), dtype=torch.int32, device=device),
                    start=torch.tensor([m, n, 0, L - 1], dtype=torch.int32, device=device),
                    workspace=words(torch, N.lightglue_adaptive_workspace_bytes(m, n, self.dim, self.num_heads), device))

    def match_adaptive(self, kpts0, kpts1, desc0, desc1, size0, size1, count0=None, count1=None, min_score: float = -1.0e30):
        """Upstream's forward pass with early stopping and point pruning, entirely on the stream.  Returns an
        ``AdaptiveMatches`` of device tensors: ``match_index`` int32 [M] and ``status`` uint8 [M] in original indices; ``scores``
        float32 [M + 1, N + 1] in compacted layout, of which rows below ``live0`` [1] and columns below ``live1`` [1] are valid, row r
        being original row ``ind0[r]`` and column c ``ind1[c]``; ``stop_layer`` int32 [1]; ``layers0`` [M] and ``layers1`` [N], the
        number of layers each original row took part in.  Every returned tensor is a buffer kept per (device, M, N): a later
        call of that size overwrites what an earlier one returned (clone what must outlive it).  Per call only the optional input
        projection and the rotary encodings are allocated, as in ``match``.  Needs ``depth_confidence`` or ``width_confidence`` > 0 at ``from_state_dict``."""
        if self._adaptive is None:
            raise ValueError("match_adaptive needs LightGlue.from_state_dict(..., depth_confidence=..., width_confidence=...) with one of them > 0")
        m, n = self._validate(kpts0, kpts1, desc0, desc1, size0, size1, count0, count1, min_score)
        depth, width, min_keypoints = self._adaptive[:3]
        L = len(self.layers)
        with OnStream(self._ctx, desc0) as on:
            torch, device = on.torch, desc0.device
            (token_w, token_b, head_w, head_b), b = self._adaptive_state(on, device, m, n)
            # the image sizes as device tensors, made once: rotary_encoding then uploads nothing, and the pass can be captured
            sizes = []
            for size in (size0, size1):
                size_key = (device, float(size[0]), float(size[1]))
                if size_key not in self._adaptive_sizes:
                    self._adaptive_sizes[size_key] = torch.as_tensor(size, dtype=torch.float32, device=device)
                sizes.append(self._adaptive_sizes[size_key])
            x0, x1, enc0, enc1 = self._inputs(on, kpts0, kpts1, desc0, desc1, sizes[0], sizes[1])
            halves, state, layers, ws = b["halves"], b["state"], b["layers"], b["workspace"]
            for dst, src in zip(halves[0], (x0, x1, enc0, enc1, b["identity"][:m], b["identity"][:n])):
                dst.copy_(src)
            state.copy_(b["start"])
            if count0 is not None:
                torch.clamp(count0, 0, m, out=state[0:1])
            if count1 is not None:
                torch.clamp(count1, 0, n, out=state[1:2])
            layers.zero_()
            live0, live1, gate = state[0:1], state[1:2], state[2:3]
            layers0, layers1 = layers[:m], layers[m:]
            d = self.dim
            for i, layer in enumerate(self.layers):
                cur, nxt = halves[i % 2], halves[(i + 1) % 2]
                if device not in layer._packed:
                    layer._packed[device] = next(iter(layer._packed.values())).to(device)
                call("ftk_transformer_layer_adaptive_device", transformer_layer_adaptive_args(
                    on.ctx, cur[0], cur[1], self.num_heads, cur[2], cur[3], layer._packed[device], live0, live1, gate, ws, on.stream), on.ctx)
                if i < L - 1:
                    call("ftk_lightglue_confidence_device", lightglue_confidence_args(
                        on.ctx, cur[0], cur[1], token_w[i], token_b[i:i + 1], head_w[i, d], head_b[i, d:d + 1], live0, live1, gate, b["conf"], b["mt"],
                        on.stream), on.ctx)
                    call("ftk_lightglue_adapt_step_device", lightglue_adapt_step_args(
                        on.ctx, self.num_heads, i, b["conf"], b["mt"], count0, count1, state, stop_threshold(i, L), depth, width, min_keypoints, cur, nxt,
                        layers0, layers1, ws, on.stream), on.ctx)
            last = halves[(L - 1) % 2]
            scores, match_index, status = b["scores"], b["match_index"], b["status"]
            call("ftk_lightglue_finish_device", lightglue_finish_args(
                on.ctx, last[0], last[1], self.num_heads, head_w, head_b, state, last[4], last[5], float(min_score), ws, scores, match_index, status,
                layers0, layers1, on.stream), on.ctx)
        return AdaptiveMatches(match_index, status, scores, last[4], last[5], live0, live1, state[3:4], layers0, layers1)


class AdaptiveMatches:
    """What ``LightGlue.match_adaptive`` returns; every field is a device tensor (see there)."""

    __slots__ = ("match_index", "status", "scores", "ind0", "ind1", "live0", "live1", "stop_layer", "layers0", "layers1")

    def __init__(self, *fields):
        for name, value in zip(self.__slots__, fields):
            setattr(self, name, value)
