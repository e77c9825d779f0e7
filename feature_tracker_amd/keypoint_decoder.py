"""``KeypointDecoder``: a SuperPoint-style network's head tensors to keypoints, scores and descriptors on the device.

The networks themselves are not part of this package.  What lies between their head tensors and what the matchers read is weight-free:
the softmax over each cell's 65 logits, the depth-to-space shuffle, suppression by distance, strongest-K selection and the bilinear
descriptor sample with its L2 normalisation.  Here that is 7 launches (10 with occupied points) on one stream, on tensors that stay where
they are: no copy to the host, no count read back, no synchronisation.  ``trim`` is the one place that synchronises.
"""
from __future__ import annotations

from . import _native as N
from ._device_keypoint_decode import check_grid, check_options, keypoint_decode_args
from ._torch_call import OnStream, PerDevice, call, check_ctx, complain, complain_cuda


class KeypointResult:
    """What one ``decode`` call leaves, all on the device: ``uv`` float32 [K, 2] ((col, row), strongest first), ``scores`` float32 [K],
    ``descriptors`` float32 [K, D] (unit length), ``count`` int32 [1]; the rows behind ``count`` are zeros.  ``heatmap`` float32 [H, W]
    when asked for."""

    __slots__ = ("uv", "scores", "descriptors", "count", "heatmap")

    def __init__(self, uv, scores, descriptors, count, heatmap=None):
        self.uv, self.scores, self.descriptors, self.count, self.heatmap = uv, scores, descriptors, count, heatmap


class KeypointDecoder:
    """``KeypointDecoder(max_keypoints=300, min_score=0.1, min_distance=20, border=4).decode(semi, desc)``.

    ``semi``: float32 CUDA [65, Hc, Wc], the detector head's logits (channel 64 the dustbin); the image is 8 Hc x 8 Wc.  ``desc``: float32
    CUDA, logically [D, Hc, Wc]: either contiguous (the network's layout) or a ``permute(2, 0, 1)`` view of a contiguous [Hc, Wc, D] tensor
    (channel-last, coalesced reads); both give the same bits.  Whatever normalisation the network applies to the coarse map is the
    caller's.  A pixel is a candidate iff its softmax score exceeds ``min_score`` and it lies at least ``border`` pixels from every image
    edge; candidates keep Chebyshev distance ``min_distance`` from each other and from the ``occupied`` points (``KltVideoTracker``'s
    rules), and the strongest ``max_keypoints`` are returned, strongest first, ties by the lower pixel index.  The
    defaults are the reference's ``NNFeaturePointDetector::Options``; ``border`` 4 is what upstream SuperPoint removes.

    Out of scope: the networks, a batch dimension, sub-pixel refinement.  Stream handling, workspace policy and capturability are
    ``TwoViewRansac``'s: the kernels run on torch's current stream (or on ``ctx``'s, from ``device.context_on_stream``), the one workspace
    per device grows to the largest call so far, and a call captured after one eager call of the same shapes allocates nothing but its
    outputs."""

    def __init__(self, max_keypoints: int = 300, min_score: float = 0.1, min_distance: int = 20, border: int = 4, ctx=None):
        self.max_keypoints, self.min_score, self.min_distance, self.border = check_options(max_keypoints, min_score, min_distance, border)
        check_ctx(ctx)
        self._ctx = ctx
        self._workspace = PerDevice()  # device -> the one workspace of this object on it, grown to the largest call so far

    def decode(self, semi, desc, occupied=None, occupied_mask=None, return_heatmap: bool = False) -> KeypointResult:
        """One image's heads to keypoints.  Everything is enqueued; the returned tensors are valid in stream order."""
        from . import device as D

        if occupied is None and occupied_mask is not None:
            raise ValueError("occupied_mask without occupied: the mask selects among the occupied points")
        tensors = [("semi", semi, D._F32, (65, None, None))]
        if occupied is not None:
            tensors.append(("occupied", occupied, D._F32, (None, 2)))
        if occupied_mask is not None:
            tensors.append(("occupied_mask", occupied_mask, D._U8, (None,)))
        complain(tensors, cuda=False)
        hc, wc = int(semi.shape[1]), int(semi.shape[2])
        check_grid(hc, wc, self.min_distance)
        # desc is [D, Hc, Wc] by its shape; its memory is that order or channel-last
        if not hasattr(desc, "permute") or len(desc.shape) != 3:
            raise ValueError(f"desc must be a float32 tensor of shape [D, {hc}, {wc}] (got {type(desc).__name__}"
                             f"{list(desc.shape) if hasattr(desc, 'shape') else ''})")
        if desc.is_contiguous():
            base, layout = desc, "chw"
        elif desc.permute(1, 2, 0).is_contiguous():
            base, layout = desc.permute(1, 2, 0), "hwc"
        else:
            raise ValueError(f"desc must be a contiguous [D, Hc, Wc] tensor or a permute(2, 0, 1) view of a contiguous [Hc, Wc, D] one (got strides "
                             f"{list(desc.stride())}); nothing is copied here")
        complain([("desc", base, D._F32, (None, hc, wc) if layout == "chw" else (hc, wc, None))], cuda=False)
        complain_cuda([(n, t) for n, t, _, _ in tensors] + [("desc", desc)])
        device = semi.device
        k, d = self.max_keypoints, int(desc.shape[0])
        n = 0 if occupied is None else int(occupied.shape[0])
        with OnStream(self._ctx, semi) as on:
            torch, ctx = on.torch, on.ctx
            workspace = self._workspace.of(torch, device, N.keypoint_decode_workspace_bytes(hc, wc, self.min_distance, n))
            f32 = dict(dtype=torch.float32, device=device)
            out = KeypointResult(torch.empty((k, 2), **f32), torch.empty(k, **f32), torch.empty((k, d), **f32),
                                 torch.empty(1, dtype=torch.int32, device=device))
            if return_heatmap:
                out.heatmap = torch.empty((8 * hc, 8 * wc), **f32)
            args = keypoint_decode_args(ctx, semi, base, k, self.min_score, self.min_distance, self.border, workspace, out.uv, out.scores, out.descriptors,
                                        out.count, out.heatmap, occupied, occupied_mask, layout, on.stream)
            call("ftk_keypoint_decode_device", args, ctx)
        return out

    @staticmethod
    def trim(result: KeypointResult) -> KeypointResult:
        """The first ``count`` rows of a result.  This is the one place that synchronises: it reads ``count``."""
        n = int(result.count.item())
        return KeypointResult(result.uv[:n], result.scores[:n], result.descriptors[:n], result.count, result.heatmap)
