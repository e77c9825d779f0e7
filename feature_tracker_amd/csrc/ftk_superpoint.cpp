// ftk_superpoint.cpp — the entry of the C ABI (include/ftk.h) that SuperPoint's forward pass adds to the conv layers of
// ftk_raft_layers.cpp: the channel-wise L2 normalisation of the dense descriptor map, written channel-last.
#include "ftk_internal.h"

extern "C" {

int ftk_channel_normalise_device(ftk_context *ctx, void *stream, const float *d_in, int32_t channels, int32_t cell_rows, int32_t cell_cols, float *d_out) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "channel_normalise_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_in || !d_out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "channel_normalise_device: null argument");
    }
    if (channels < 1 || channels > FTK_KEYPOINT_DECODE_MAX_CHANNELS) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "channel_normalise_device: channels %d outside 1 .. FTK_KEYPOINT_DECODE_MAX_CHANNELS = %d", channels,
                        FTK_KEYPOINT_DECODE_MAX_CHANNELS);
    }
    if (cell_rows < 1 || cell_cols < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "channel_normalise_device: sizes %d x %d must be positive", cell_rows, cell_cols);
    }
    const int64_t cells = (int64_t)cell_rows * cell_cols;  // below 2^62; times 4 * FTK_KEYPOINT_DECODE_MAX_CHANNELS below 2^63
    if ((cells + 63) / 64 > 0x7fffffff) {  // channel_normalise_launch's grid: 64 cells per workgroup
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "channel_normalise_device: %d x %d cells do not fit a launch", cell_rows, cell_cols);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::channel_normalise_launch(d_in, d_out, channels, cells, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
