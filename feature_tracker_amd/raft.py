"""RAFT's two operators that are not stock torch layers: the correlation pyramid (src/nn_optical_flow_tracker/raft/
correlation_volumes.py:19-83) as a drop-in class, and the convex flow upsampling (Raft.UpsampleFlow, model.py:48-64) as a function.

``CorrelationPyramid(fmap0, fmap1, num_levels, radius)`` keeps the reference's attributes (``num_levels``, ``radius``,
``correlation_pyramid``) and ``__call__``; ``lookup`` returns the fused ``[B, L*K, H, W]`` tensor that model.py:87-88 builds with
``cat`` / ``permute`` / ``contiguous``.  torch owns every buffer (one volume tensor, the levels are views into it) and the kernels
launch on ``torch.cuda.current_stream()`` at each call, so construction and lookups can be captured in ``torch.cuda.graph``.
``upsample_flow(flow, mask, mask_scale)`` is ``Raft.UpsampleFlow(flow, mask_scale * mask)`` in one launch.
Inference only, float32 only, and no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Dict, List

from . import _native as N
from . import device as D
from .tracker import Context

_contexts: Dict[int, Context] = {}


def _context(index: int) -> Context:
    """One library context per device: it selects the device and records errors; the launches go to torch's current stream."""
    ctx = _contexts.get(index)
    if ctx is None:
        ctx = _contexts[index] = Context(index)
    return ctx


def _check_no_grad(torch, *tensors, what: str = "CorrelationPyramid") -> None:
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError(f"{what} is inference only (no backward): run it under torch.no_grad() or pass tensors that do not "
                           "require grad")


class CorrelationPyramid:
    """correlation_volumes.py:19-34: the all-pairs correlation of two float32 CUDA feature maps [B, C, H, W] and its
    ``num_levels - 1`` 2x2 average pools, built on the device by the HIP kernels of raft_corr_kernels.hip."""

    def __init__(self, fmap0, fmap1, num_levels: int, radius: int):
        torch = D._torch()
        for name, t in (("fmap0", fmap0), ("fmap1", fmap1)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 4:
                raise ValueError(f"{name} must be a 4-D float32 CUDA tensor [B, C, H, W] (no CPU fallback, no other dtype)")
        if fmap0.size() != fmap1.size() or fmap0.device != fmap1.device:
            raise ValueError(f"fmap0 and fmap1 must have the same size and device: {tuple(fmap0.shape)} on {fmap0.device} vs "
                             f"{tuple(fmap1.shape)} on {fmap1.device}")
        _check_no_grad(torch, fmap0, fmap1)
        if not 0 <= int(radius) <= N.FTK_CORR_MAX_RADIUS:
            raise ValueError(f"radius {radius} outside 0 .. {N.FTK_CORR_MAX_RADIUS}")
        B, _, H, W = fmap0.shape
        try:
            elements, offsets, dims = N.corr_pyramid_layout(B, H, W, int(num_levels))
        except N.FtkError as e:
            raise ValueError(f"CorrelationPyramid of {H} x {W} feature maps with num_levels={num_levels}: {e}") from None
        self.num_levels = int(num_levels)
        self.radius = int(radius)
        self._shape = (B, H, W)
        self._device = fmap0.device
        self._ctx = _context(fmap0.device.index if fmap0.device.index is not None else torch.cuda.current_device())
        self._volume = torch.empty(elements, dtype=torch.float32, device=fmap0.device)
        D.corr_pyramid_build_device(self._ctx, fmap0.contiguous(), fmap1.contiguous(), self.num_levels, self._volume)
        n = B * H * W
        # the reference's list of [B*H*W, 1, H_l, W_l] tensors: zero-copy views into the one volume
        self.correlation_pyramid: List = [self._volume[off:off + n * h * w].view(n, 1, h, w) for off, (h, w) in zip(offsets, dims)]

    def _coords(self, pixel_locations):
        torch = D._torch()
        if not isinstance(pixel_locations, torch.Tensor) or pixel_locations.dim() != 4 or pixel_locations.size(1) != 2:
            raise ValueError("The size of pixel_locations should be [batch_size, 2, height, width].")
        B, H, W = self._shape
        if tuple(pixel_locations.shape) != (B, 2, H, W):
            raise ValueError(f"pixel_locations must be [{B}, 2, {H}, {W}] for this pyramid (got {tuple(pixel_locations.shape)})")
        if pixel_locations.dtype != torch.float32 or pixel_locations.device != self._device:
            raise ValueError(f"pixel_locations must be float32 on {self._device} (got {pixel_locations.dtype} on {pixel_locations.device})")
        _check_no_grad(torch, pixel_locations)
        return pixel_locations.contiguous()

    def __call__(self, pixel_locations):
        """correlation_volumes.py:48-77: per level a contiguous [B, H, W, (2r+1)^2] tensor of the bilinear window samples."""
        torch = D._torch()
        coords = self._coords(pixel_locations)
        B, H, W = self._shape
        K = (2 * self.radius + 1) ** 2
        block = B * H * W * K
        out = torch.empty(self.num_levels * block, dtype=torch.float32, device=self._device)
        D.corr_pyramid_lookup_device(self._ctx, self._volume, self.num_levels, self.radius, coords, out, per_level=True)
        return [out[l * block:(l + 1) * block].view(B, H, W, K) for l in range(self.num_levels)]

    def lookup(self, pixel_locations):
        """``torch.cat(self(pixel_locations), -1).permute(0, 3, 1, 2).contiguous()`` (model.py:87-88) in one launch: [B, L*K, H, W]."""
        torch = D._torch()
        coords = self._coords(pixel_locations)
        B, H, W = self._shape
        K = (2 * self.radius + 1) ** 2
        out = torch.empty((B, self.num_levels * K, H, W), dtype=torch.float32, device=self._device)
        D.corr_pyramid_lookup_device(self._ctx, self._volume, self.num_levels, self.radius, coords, out, per_level=False)
        return out


def upsample_flow(flow, mask, mask_scale: float = 1.0):
    """``Raft.UpsampleFlow(flow, mask_scale * mask)`` (model.py:48-64; update_block.py:66 is the 0.25 that ``mask_scale`` folds in):
    ``flow`` [B, 2, H, W] and ``mask`` [B, 576, H, W], float32 CUDA tensors, give a new [B, 2, 8H, 8W] tensor — per fine pixel the
    softmax of its 9 logits applied to 8 * flow of the zero-padded 3 x 3 coarse neighbourhood, by one HIP kernel
    (raft_upsample_kernels.hip) on torch's current stream.  ``B`` is just the leading dimension: the flows and masks of T iterations
    stacked as [T * B, ...] take one call.  Arguments are checked before any device is touched."""
    import torch

    for name, t, channels in (("flow", flow, 2), ("mask", mask, 576)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.size(1) != channels:
            got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{name} must be a 4-D float32 CUDA tensor [B, {channels}, H, W] (no CPU fallback, no other dtype): got {got}")
    B, _, H, W = flow.shape
    if tuple(mask.shape) != (B, 576, H, W) or flow.device != mask.device:
        raise ValueError(f"flow and mask must agree in B, H, W and device: {tuple(flow.shape)} on {flow.device} vs {tuple(mask.shape)} on "
                         f"{mask.device}")
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"flow must not be empty (got {tuple(flow.shape)})")
    if not math.isfinite(float(mask_scale)):
        raise ValueError(f"mask_scale must be finite (got {mask_scale})")
    if not flow.is_cuda:
        raise ValueError(f"flow and mask must be CUDA tensors (got them on {flow.device}): there is no CPU fallback")
    _check_no_grad(torch, flow, mask, what="upsample_flow")
    torch = D._torch()
    ctx = _context(flow.device.index if flow.device.index is not None else torch.cuda.current_device())
    out = torch.empty((B, 2, 8 * H, 8 * W), dtype=torch.float32, device=flow.device)
    D.flow_upsample_device(ctx, flow.contiguous(), mask.contiguous(), out, mask_scale)
    return out
