// ftk_flow_warm.cpp — the warm start of RAFT on video of the C ABI (include/ftk.h): a coarse flow pushed forward along itself, in place of
// upstream RAFT's forward_interpolate (core/utils/utils.py), which does it on the host with scipy's griddata(method="nearest")
// (DESIGN.md 5.18).
#include "ftk_internal.h"

static_assert(FTK_FLOW_WARM_MAX_PIXELS == ftk::kFlowWarmMaxPixels && FTK_FLOW_WARM_MAX_SPLITS == ftk::kFlowWarmMaxSplits, "include/ftk.h states the limits");

extern "C" {

int ftk_flow_warm_splits(int32_t B, int32_t H, int32_t W, int32_t *splits) {
    if (!splits) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "flow_warm_splits: null argument");
    }
    if (B < 1 || H < 1 || W < 1) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "flow_warm_splits: sizes B %d, H %d, W %d must be positive", B, H, W);
    }
    if ((int64_t)H * W > FTK_FLOW_WARM_MAX_PIXELS) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "flow_warm_splits: %d x %d pixels above FTK_FLOW_WARM_MAX_PIXELS = %d: the search is exhaustive", H,
                        W, FTK_FLOW_WARM_MAX_PIXELS);
    }
    *splits = ftk::flow_warm_auto_splits(B, H, W);
    return FTK_OK;
}

int ftk_flow_warm_device(ftk_context *ctx, void *stream, const float *d_flow, int32_t B, int32_t H, int32_t W, int32_t splits,
                         uint64_t *d_workspace, float *d_out) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "flow_warm_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_flow || !d_out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_warm_device: null argument");
    }
    if (static_cast<const void *>(d_flow) == static_cast<const void *>(d_out)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_warm_device: d_out is d_flow: every target reads sources all over the input");
    }
    if (B < 1 || H < 1 || W < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_warm_device: sizes B %d, H %d, W %d must be positive", B, H, W);
    }
    if ((int64_t)H * W > FTK_FLOW_WARM_MAX_PIXELS) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_warm_device: %d x %d pixels above FTK_FLOW_WARM_MAX_PIXELS = %d: the search is exhaustive", H, W,
                        FTK_FLOW_WARM_MAX_PIXELS);
    }
    if (splits < 1 || splits > FTK_FLOW_WARM_MAX_SPLITS) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_warm_device: splits %d outside 1 .. %d", splits, FTK_FLOW_WARM_MAX_SPLITS);
    }
    if (splits > 1 && !d_workspace) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_warm_device: %d splits need a workspace of splits * B * H * W 64-bit words", splits);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    ftk::FlowWarmParams p{};
    p.flow = d_flow;
    p.workspace = reinterpret_cast<unsigned long long *>(d_workspace);
    p.out = d_out;
    p.B = B;
    p.H = H;
    p.W = W;
    p.splits = splits;
    FTK_HIP(ctx, ftk::flow_warm_launch(p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
