"""``MatchAssignment``: LightGlue's assignment head on the device.

The last stage of LightGlue, and the producer of the tensor ``NNFeatureMatcher`` reads: two ``Linear`` layers, the M x N similarity, a
log-softmax along both axes, the matchability terms and the dustbin row and column.  The transformer layers before it are
``TransformerLayer`` (transformer.py); ``LightGlue`` composes them with this head.  Without weights the same kernels are the dual-softmax matcher of LoFTR-style pipelines, which takes ``KeypointDecoder``'s
descriptors as they are.  4 launches (3 without weights) on one stream, on tensors that stay where they are: no copy to the host, no
count read back, no synchronisation.
"""
from __future__ import annotations

from . import _native as N
from ._device_match_assignment import check_row_stride, check_scale, check_sizes, match_assignment_args
from ._torch_call import OnStream, PerKey, call, check_ctx, complain, complain_cuda, words

_KEYS = ("final_proj.weight", "final_proj.bias", "matchability.weight", "matchability.bias")


class MatchAssignment:
    """``MatchAssignment.from_state_dict(sd)`` or ``MatchAssignment.without_weights(dim)``, then ``assign(desc0, desc1)`` or ``match(...)``.

    ``desc0``: float32 CUDA [M, D], ``desc1``: [N, D], contiguous.  ``count0`` / ``count1``: optional int32 [1] device tensors
    (``KeypointDecoder``'s ``count``): only the first ``clamp(count, 0, rows)`` rows of that side are valid; they are read on the device.
    ``assign`` returns ``scores`` float32 [M + 1, N + 1], laid out like upstream's tensor with the dustbin row and column last: entry
    (i, j) is ``log_softmax(sim, 1) + log_softmax(sim, 0) + logsigmoid(z0_i) + logsigmoid(z1_j)`` over the valid block, the dustbins
    ``logsigmoid(-z)``, the corner 0; every entry of an invalid row or column is -inf.  Without weights there is no ``z``: the dustbins
    are -inf too.  The bits are those of DESIGN.md 5.23's contract, which the tests hold to a scalar restatement.

    Limits: 1 <= M, N <= 4 096, 1 <= D <= 1 024, float32, one pair per call.  Out of scope: a batch dimension,
    upstream's ``filter_matches`` threshold on ``exp(score)`` (``NNFeatureMatcher`` thresholds the log score).  The kernels run on torch's
    current stream (or on ``ctx``'s, from ``device.context_on_stream``); the object keeps one workspace per (device, M, N), so a call
    captured after one eager call at that size allocates nothing but its outputs.  There is no CPU fallback."""

    def __init__(self, dim: int, packed_weights=None, packed_bias=None, scale=None, ctx=None):
        if isinstance(dim, bool) or not isinstance(dim, int) or not 1 <= dim <= N.FTK_MATCH_ASSIGNMENT_MAX_DIM:
            raise ValueError(f"dim must be an integer in 1 .. FTK_MATCH_ASSIGNMENT_MAX_DIM = {N.FTK_MATCH_ASSIGNMENT_MAX_DIM} (got {dim!r})")
        check_ctx(ctx)
        self.dim = dim
        self.with_weights = packed_weights is not None
        self.scale = 1.0 if self.with_weights else check_scale(dim ** -0.25 if scale is None else scale)
        self._packed = {} if packed_weights is None else {packed_weights.device: (packed_weights, packed_bias)}
        self._ctx = ctx
        self._workspace = PerKey()  # (device, M, N) -> the workspace of that size

    @classmethod
    def from_state_dict(cls, sd, prefix: str = "log_assignment.8.", ctx=None) -> "MatchAssignment":
        """Upstream LightGlue's four tensors ``{prefix}final_proj.weight`` [D, D], ``final_proj.bias`` [D], ``matchability.weight`` [1, D]
        and ``matchability.bias`` [1], packed once as [D + 1, D] and [D + 1].  ``D`` is read off the weights."""
        import torch

        missing = [k for k in _KEYS if prefix + k not in sd]
        if missing:
            raise ValueError(f"the state dict lacks {[prefix + k for k in missing]}")
        pw, pb, mw, mb = (sd[prefix + k] for k in _KEYS)
        for k, t in zip(_KEYS, (pw, pb, mw, mb)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise ValueError(f"{prefix}{k} must be a float32 tensor (got {getattr(t, 'dtype', type(t).__name__)})")
        if pw.dim() != 2 or pw.shape[0] != pw.shape[1]:
            raise ValueError(f"{prefix}final_proj.weight must be [D, D] (got {list(pw.shape)})")
        d = int(pw.shape[0])
        for k, t, shape in zip(_KEYS[1:], (pb, mw, mb), ((d,), (1, d), (1,))):
            if tuple(t.shape) != shape:
                raise ValueError(f"{prefix}{k} must be {list(shape)} (got {list(t.shape)})")
        if not 1 <= d <= N.FTK_MATCH_ASSIGNMENT_MAX_DIM:
            raise ValueError(f"D must be in 1 .. FTK_MATCH_ASSIGNMENT_MAX_DIM = {N.FTK_MATCH_ASSIGNMENT_MAX_DIM} (got {d})")
        weights = torch.cat([pw.detach(), mw.detach().to(pw.device)], 0).contiguous()
        bias = torch.cat([pb.detach().to(pw.device), mb.detach().to(pw.device)], 0).contiguous()
        return cls(d, weights, bias, None, ctx)

    @classmethod
    def without_weights(cls, dim: int, scale=None, ctx=None) -> "MatchAssignment":
        """No projection and no matchability: ``sim = (desc0 * scale) @ (desc1 * scale).T``; ``scale`` defaults to upstream's
        ``dim ** -0.25`` per side."""
        return cls(dim, None, None, scale, ctx)

    # ---- the calls ----

    def _validate(self, desc0, desc1, count0, count1, out, row_stride):
        from . import device as D

        tensors = [("desc0", desc0, D._F32, (None, self.dim)), ("desc1", desc1, D._F32, (None, self.dim))]
        if count0 is not None:
            tensors.append(("count0", count0, D._I32, (1,)))
        if count1 is not None:
            tensors.append(("count1", count1, D._I32, (1,)))
        complain(tensors, cuda=False)
        m, n = int(desc0.shape[0]), int(desc1.shape[0])
        check_sizes(m, n, self.dim)
        if out is not None:
            if not hasattr(out, "data_ptr") or str(out.dtype) != "torch.float32" or tuple(out.shape) != (m + 1, n + 1) or out.stride(1) != 1:
                raise ValueError(f"out must be a float32 tensor of shape [{m + 1}, {n + 1}] with unit column stride (got "
                                 f"{getattr(out, 'dtype', type(out).__name__)} {list(getattr(out, 'shape', []))})")
            if row_stride is not None and row_stride != out.stride(0):
                raise ValueError(f"row_stride {row_stride} is not out's row stride {out.stride(0)}")
            row_stride = int(out.stride(0))
            tensors.append(("out", out, None, None))
        stride = check_row_stride(row_stride, n)
        complain_cuda((name, t) for name, t, _, _ in tensors)
        return m, n, stride

    def assign(self, desc0, desc1, count0=None, count1=None, out=None, row_stride=None):
        """``scores`` float32 [M + 1, N + 1] (a view of M + 1 rows of ``row_stride`` floats when that is given: padding behind N + 1 is
        left untouched).  Everything is enqueued; the tensor is valid in stream order."""
        m, n, stride = self._validate(desc0, desc1, count0, count1, out, row_stride)
        return self._run(desc0, desc1, count0, count1, out, m, n, stride, None)

    def match(self, desc0, desc1, count0=None, count1=None, out=None, row_stride=None, min_score: float = -1.0e30):
        """``assign``, then ``nn_match_scores_device`` on the [:M, :N] view: ``(scores, match_index int32 [M], status uint8 [M])``.
        ``min_score`` is a threshold on the log score, as ``NNFeatureMatcher``'s.  Nothing is read back."""
        import math

        if isinstance(min_score, bool) or not isinstance(min_score, (int, float)) or math.isnan(min_score):
            raise ValueError(f"min_score must be a number (got {min_score!r})")
        m, n, stride = self._validate(desc0, desc1, count0, count1, out, row_stride)
        return self._run(desc0, desc1, count0, count1, out, m, n, stride, float(min_score))

    def _run(self, desc0, desc1, count0, count1, out, m, n, stride, min_score):
        from . import device as D

        device = desc0.device
        with OnStream(self._ctx, desc0) as on:
            torch, ctx, stream = on.torch, on.ctx, on.stream
            weights = bias = None
            if self.with_weights:
                if device not in self._packed:
                    w, b = next(iter(self._packed.values()))
                    self._packed[device] = (w.to(device), b.to(device))
                weights, bias = self._packed[device]
            workspace = self._workspace.of((device, m, n), lambda: words(torch, N.match_assignment_workspace_bytes(m, n, self.dim, self.with_weights), device))
            if out is None:
                flat = torch.empty((m + 1) * stride, dtype=torch.float32, device=device)
                scores = flat.as_strided((m + 1, n + 1), (stride, 1))
            else:
                scores = out
                flat = out.as_strided((m * stride + n + 1,), (1,))
            call("ftk_match_assignment_device", match_assignment_args(ctx, desc0, desc1, weights, bias, self.scale, count0, count1, workspace, flat, stride, stream),
                 ctx)
            result = scores
            if min_score is not None:
                match_index = torch.empty((1, m), dtype=torch.int32, device=device)
                status = torch.empty((1, m), dtype=torch.uint8, device=device)
                D.nn_match_scores_device(ctx, scores[:m, :n].unsqueeze(0), min_score, match_index, status, stream)
                result = (scores, match_index[0], status[0])
        return result
