"""NNFeatureMatcher (src/nn_feature_matcher/nn_feature_matcher.{h,cpp}): everything ``Match`` does AFTER the network (:155-216).

The LightGlue network itself is not part of this project (it needs an ONNX runtime and model files the reference does not ship):
callers run it where they like — typically in torch on the same device — and hand its output here:

* score-matrix models (``kLightglueFor*ScoreMat``): ``match_scores(scores)`` — per-column and per-row first argmax, the score
  threshold, the mutual check (:177-215), in one read of the matrix;
* match-list models (``kLightglueFor*Matches``): ``match_list(matches, n_ref, n_cur)`` — the bounds-checked scatter in which a later
  row overrides an earlier one (:158-174).

Both return ``(ok, match_index, status)`` — ``match_index[i]`` the matched column or -1, ``status[i]`` ``TRACKED`` or ``LARGE_RESIDUAL``
(:156) — plus ``matched_uv`` when ``uv_cur`` is given: a copy of ``uv_cur`` (n_cur entries, :157) whose entry ``i`` is
``uv_cur[match_index[i]]`` for matched rows.  torch CUDA tensors run on torch's current stream without synchronisation or allocation
by the library (usable inside ``torch.cuda.graph`` once one call of the size has been made outside it); numpy arrays go through the
synchronous host entries.  Inference only, float32 scores only, no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _native as N
from . import device as D
from ._torch_call import context_of_index
from .tracker import Context, _ptr, default_context


class NNFeatureMatcherOptions:
    """nn_feature_matcher.h:16-27.  ``kMaxNumberOfMatches`` only sizes the reference's warm-up inference (:57-70) and has no effect
    on ``Match``: it is carried for source compatibility and unused here.  ``kModelType`` names the model whose output the caller
    passes; it does not change the arithmetic (the caller picks ``match_scores`` or ``match_list``)."""

    kLightglueForSuperpointScoreMat, kLightglueForSuperpointMatches, kLightglueForDiskScoreMat, kLightglueForDiskMatches = range(4)

    def __init__(self):
        self.kMaxNumberOfMatches = 300
        self.kMinValidMatchScore = -3.0
        self.kModelType = self.kLightglueForSuperpointScoreMat


def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _fill_host(match_index: np.ndarray, uv_cur: np.ndarray) -> np.ndarray:
    """The pixel fill on host arrays (:157, :171, :213): an index gather over n_cur entries; rows >= n_cur keep their index and
    status and write no pixel."""
    n_cur = uv_cur.shape[0]
    matched = uv_cur.copy()
    idx = match_index[:n_cur]
    rows = np.nonzero((idx >= 0) & (idx < n_cur))[0]
    matched[rows] = uv_cur[idx[rows]]
    return matched


class NNFeatureMatcher:
    """The post-processing of NNFeatureMatcher::Match on the device (nn_match_kernels.hip)."""

    ModelType = NNFeatureMatcherOptions

    def __init__(self, ctx: Optional[Context] = None):
        self._ctx = ctx
        self._options = NNFeatureMatcherOptions()

    def options(self) -> NNFeatureMatcherOptions:
        return self._options

    def _context(self, device_index: Optional[int] = None) -> Context:
        if self._ctx is not None:
            return self._ctx
        if device_index is None:
            return default_context()
        return context_of_index(device_index)  # one library context per torch device

    # ---- score-matrix models ----

    def match_scores(self, scores, uv_ref=None, uv_cur=None):
        """scores: float32 [n_ref, n_cur] or [B, n_ref, n_cur] with unit column stride (pass ``log_assignment[:, :-1, :-1]`` to leave
        LightGlue's dustbins out).  Returns (ok, match_index, status[, matched_uv]); ok is False for n_ref == 0 (:92) or when the
        sizes of uv_ref / uv_cur do not fit the matrix (:93)."""
        if _is_tensor(scores):
            return self._match_scores_torch(scores, uv_ref, uv_cur)
        s = np.asarray(scores)
        if s.dtype != np.float32 or s.ndim not in (2, 3):
            raise ValueError("scores must be a float32 array [n_ref, n_cur] or [B, n_ref, n_cur]")
        batched = s.ndim == 3
        s3 = s if batched else s[None]
        B, n_ref, n_cur = s3.shape
        if n_cur > 1 and s3.strides[2] != 4:
            s3 = np.ascontiguousarray(s3)
        if any(st % 4 or st < 0 for st in s3.strides):
            s3 = np.ascontiguousarray(s3)
        uv = None if uv_cur is None else np.ascontiguousarray(uv_cur, dtype=np.float32).reshape(B, -1, 2) if batched else \
            np.ascontiguousarray(uv_cur, dtype=np.float32).reshape(1, -1, 2)
        if n_ref == 0 or (uv is not None and uv.shape[1] != n_cur) or (uv_ref is not None and np.asarray(uv_ref).reshape(B, -1, 2).shape[1] != n_ref):
            return (False, None, None) + ((None,) if uv_cur is not None else ())
        ctx = self._context()
        idx = np.empty((B, n_ref), np.int32)
        st = np.empty((B, n_ref), np.uint8)
        ok = C.c_int(0)
        row_stride = s3.strides[1] // 4 if n_ref > 1 else max(n_cur, 1)
        batch_stride = s3.strides[0] // 4 if B > 1 else 0
        rc = N.lib().ftk_nn_match_scores(ctx.handle, C.c_void_p(s3.ctypes.data), B, n_ref, n_cur, row_stride, batch_stride,
                                         float(self._options.kMinValidMatchScore), _ptr(idx), _ptr(st), C.byref(ok))
        N.check(rc, ctx.handle)
        out = (bool(ok.value), idx if batched else idx[0], st if batched else st[0])
        if uv_cur is not None:
            m = np.stack([_fill_host(idx[b], uv[b]) for b in range(B)])
            out += (m if batched else m[0],)
        return out

    def _match_scores_torch(self, scores, uv_ref, uv_cur):
        torch = D._torch()
        if scores.dim() not in (2, 3):
            raise ValueError("scores must be [n_ref, n_cur] or [B, n_ref, n_cur]")
        if torch.is_grad_enabled() and scores.requires_grad:
            raise RuntimeError("NNFeatureMatcher is inference only (no backward): run it under torch.no_grad() or detach the scores")
        batched = scores.dim() == 3
        s3 = scores if batched else scores.unsqueeze(0)
        B, n_ref, n_cur = s3.shape
        uv = None
        if uv_cur is not None:
            uv = uv_cur if batched else uv_cur.unsqueeze(0)
            if uv.dtype != torch.float32 or uv.device != scores.device or uv.dim() != 3 or uv.size(0) != B or uv.size(2) != 2:
                raise ValueError("uv_cur must be a float32 tensor [n_cur, 2] (or [B, n_cur, 2]) on the scores' device")
        if n_ref == 0 or (uv is not None and uv.size(1) != n_cur) or (uv_ref is not None and uv_ref.reshape(B, -1, 2).size(1) != n_ref):
            return (False, None, None) + ((None,) if uv_cur is not None else ())
        ctx = self._context(scores.device.index if scores.device.index is not None else torch.cuda.current_device())
        idx = torch.empty((B, n_ref), dtype=torch.int32, device=scores.device)
        st = torch.empty((B, n_ref), dtype=torch.uint8, device=scores.device)
        D.nn_match_scores_device(ctx, s3, self._options.kMinValidMatchScore, idx, st)
        out = (True, idx if batched else idx[0], st if batched else st[0])
        if uv is not None:
            uv = uv.contiguous()
            m = torch.empty_like(uv)
            for b in range(B):
                D.nn_fill_pixels_device(ctx, idx[b], uv[b], m[b])
            out += (m if batched else m[0],)
        return out

    # ---- match-list models ----

    def match_list(self, matches, n_ref: int, n_cur: int, uv_cur=None):
        """matches: int64 [K, 2] rows of (idx_ref, idx_cur).  A row is applied iff 0 <= idx_ref < min(n_ref, n_cur) and
        0 <= idx_cur < n_cur; the last applied row of an idx_ref wins.  Returns (ok, match_index, status[, matched_uv])."""
        n_ref, n_cur = int(n_ref), int(n_cur)
        if n_ref < 0 or n_cur < 0:
            raise ValueError(f"negative size (n_ref {n_ref}, n_cur {n_cur})")
        if _is_tensor(matches):
            torch = D._torch()
            if uv_cur is not None and (uv_cur.dtype != torch.float32 or uv_cur.device != matches.device or tuple(uv_cur.shape) != (n_cur, 2)):
                raise ValueError(f"uv_cur must be a float32 tensor [{n_cur}, 2] on the matches' device")
            if n_ref == 0:
                return (False, None, None) + ((None,) if uv_cur is not None else ())
            ctx = self._context(matches.device.index if matches.device.index is not None else torch.cuda.current_device())
            idx = torch.empty(n_ref, dtype=torch.int32, device=matches.device)
            st = torch.empty(n_ref, dtype=torch.uint8, device=matches.device)
            D.nn_match_list_device(ctx, matches, n_ref, n_cur, idx, st)
            out = (True, idx, st)
            if uv_cur is not None:
                uv = uv_cur.contiguous()
                m = torch.empty_like(uv)
                if n_cur > 0:
                    D.nn_fill_pixels_device(ctx, idx, uv, m)
                out += (m,)
            return out
        mt = np.ascontiguousarray(matches, dtype=np.int64).reshape(-1, 2)
        uv = None if uv_cur is None else np.ascontiguousarray(uv_cur, dtype=np.float32).reshape(-1, 2)
        if uv is not None and uv.shape[0] != n_cur:
            raise ValueError(f"uv_cur must have n_cur = {n_cur} entries")
        if n_ref == 0:
            return (False, None, None) + ((None,) if uv_cur is not None else ())
        ctx = self._context()
        idx = np.empty(n_ref, np.int32)
        st = np.empty(n_ref, np.uint8)
        ok = C.c_int(0)
        rc = N.lib().ftk_nn_match_list(ctx.handle, _ptr(mt), mt.shape[0], n_ref, n_cur, _ptr(idx), _ptr(st), C.byref(ok))
        N.check(rc, ctx.handle)
        out = (bool(ok.value), idx, st)
        if uv is not None:
            out += (_fill_host(idx, uv),)
        return out
