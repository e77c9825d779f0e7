// ftk_pyramid.cpp — image pyramids of the C ABI (include/ftk.h): upload, wrap, build / update on the device, download.
#include <string.h>

#include <new>

#include "ftk_internal.h"

namespace {

int make_pyramid(ftk_context *ctx, ftk_pyramid **out) {
    if (!ctx || !out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid: null context or output");
    }
    ftk_pyramid *pyr = new (std::nothrow) ftk_pyramid();
    if (!pyr) {
        return ftk_fail(ctx, FTK_E_OUT_OF_MEMORY, "pyramid: host allocation failed");
    }
    pyr->device = ctx->device;
    *out = pyr;
    return FTK_OK;
}

// The trackers index a level with 32-bit pixel offsets formed on the 24-bit multiplier (klt_scalar.h px()).
bool level_addressable(int32_t rows, int32_t cols) { return rows < (1 << 24) && cols < (1 << 24) && (long long)rows * cols < (1ll << 32); }

int check_levels(ftk_context *ctx, const ftk_image *levels, int32_t n_levels) {
    if (!levels || n_levels < 1 || n_levels > FTK_MAX_LEVELS) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid: n_levels %d outside [1, %d]", n_levels, FTK_MAX_LEVELS);
    }
    for (int i = 0; i < n_levels; ++i) {
        if (!levels[i].data || levels[i].rows <= 0 || levels[i].cols <= 0) {
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid: level %d is empty", i);
        }
        if (!level_addressable(levels[i].rows, levels[i].cols)) {
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "pyramid: level %d (%d x %d) exceeds 2^24 on a side or 2^32 pixels", i, levels[i].rows, levels[i].cols);
        }
    }
    return FTK_OK;
}

}  // namespace

int ftk_acquire_image_stage(ftk_context *ctx, size_t bytes, ftk_context::ImageStage **out) {
    *out = nullptr;
    ftk_context::ImageStage &st = ctx->image_stage[ctx->image_stage_next];
    if (st.busy) {
        FTK_HIP(ctx, hipEventSynchronize(st.done));  // normally long past: two frames per tracker call
        st.busy = false;
    }
    bool grew = false;
    FTK_HIP(ctx, st.host.reserve(ctx->stream, bytes, 0, 1u << 20, &grew));
    if (grew) {
        void *d = nullptr;
        if (hipHostGetDevicePointer(&d, st.host.get(), 0) != hipSuccess || d == nullptr) {
            (void)hipGetLastError();
            st.host.release();
            return FTK_OK;  // *out == nullptr
        }
        st.device_view = static_cast<const uint8_t *>(d);
    }
    if (!st.done) {
        FTK_HIP(ctx, hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    }
    ctx->image_stage_next ^= 1;
    *out = &st;
    return FTK_OK;
}

extern "C" {

int ftk_pyramid_upload(ftk_context *ctx, const ftk_image *host_levels, int32_t n_levels, ftk_pyramid **out) {
    FTK_TRACE_SCOPE("ftk_pyramid_upload");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "pyramid_upload: null context");
    }
    FTK_LOCK(ctx);
    int rc = check_levels(ctx, host_levels, n_levels);
    if (rc != FTK_OK) {
        return rc;
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    ftk_layout L;  // of the pyramid's own block and of its image in the pinned block
    ftk_slot<uint8_t> slots[FTK_MAX_LEVELS];
    for (int i = 0; i < n_levels; ++i) {
        slots[i] = L.take<uint8_t>((size_t)host_levels[i].rows * host_levels[i].cols);
    }
    if (!L.ok()) {
        return ftk_layout_refused(ctx);
    }
    const size_t total = L.bytes();
    ftk_pyramid *pyr = nullptr;
    rc = make_pyramid(ctx, &pyr);
    if (rc != FTK_OK) {
        return rc;
    }
    hipError_t e = pyr->owned.reserve(ctx->stream, total, 0, 1);
    if (e != hipSuccess) {
        delete pyr;
        return ftk_fail(ctx, FTK_E_OUT_OF_MEMORY, "pyramid_upload: device allocation of %zu bytes failed: %s", total, hipGetErrorString(e));
    }
    pyr->n_levels = n_levels;
    // gather the levels in pinned staging, then ONE H2D copy of the whole pyramid
    if (ftk_ensure_pinned(ctx, total) != FTK_OK) {
        ftk_pyramid_destroy(pyr);
        return FTK_E_OUT_OF_MEMORY;
    }
    uint8_t *staging = ctx->pinned.as<uint8_t>(), *owned = pyr->owned.as<uint8_t>();
    for (int i = 0; i < n_levels; ++i) {
        memcpy(slots[i].in(staging), host_levels[i].data, slots[i].size_bytes());
        pyr->levels[i].data = slots[i].in(owned);
        pyr->levels[i].rows = host_levels[i].rows;
        pyr->levels[i].cols = host_levels[i].cols;
    }
    e = hipMemcpyAsync(owned, staging, total, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        e = hipStreamSynchronize(ctx->stream);  // staging and the caller's buffers are free again on return
    }
    if (e != hipSuccess) {
        ftk_pyramid_destroy(pyr);
        return ftk_fail(ctx, FTK_E_HIP, "pyramid_upload: copy failed: %s", hipGetErrorString(e));
    }
    *out = pyr;
    return FTK_OK;
}

int ftk_pyramid_wrap_device(ftk_context *ctx, const ftk_image *device_levels, int32_t n_levels, ftk_pyramid **out) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "pyramid_wrap_device: null context");
    }
    FTK_LOCK(ctx);
    int rc = check_levels(ctx, device_levels, n_levels);
    if (rc != FTK_OK) {
        return rc;
    }
    ftk_pyramid *pyr = nullptr;
    rc = make_pyramid(ctx, &pyr);
    if (rc != FTK_OK) {
        return rc;
    }
    pyr->n_levels = n_levels;
    for (int i = 0; i < n_levels; ++i) {
        pyr->levels[i].data = device_levels[i].data;
        pyr->levels[i].rows = device_levels[i].rows;
        pyr->levels[i].cols = device_levels[i].cols;
    }
    *out = pyr;
    return FTK_OK;
}

int ftk_pyramid_build(ftk_context *ctx, const uint8_t *image, int32_t rows, int32_t cols, int32_t n_levels, int image_on_device,
                      ftk_pyramid **out) {
    FTK_TRACE_SCOPE("ftk_pyramid_build");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "pyramid_build: null context");
    }
    FTK_LOCK(ctx);
    if (!image || rows <= 0 || cols <= 0 || n_levels < 1 || n_levels > FTK_MAX_LEVELS || !out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid_build: bad image or level count");
    }
    if (!level_addressable(rows, cols)) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "pyramid_build: image %d x %d exceeds 2^24 on a side or 2^32 pixels", rows, cols);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    int32_t lrows[FTK_MAX_LEVELS], lcols[FTK_MAX_LEVELS];
    ftk_layout L;
    ftk_slot<uint8_t> slots[FTK_MAX_LEVELS];
    lrows[0] = rows;
    lcols[0] = cols;
    for (int i = 0; i < n_levels; ++i) {
        if (i > 0) {
            lrows[i] = lrows[i - 1] / 2;
            lcols[i] = lcols[i - 1] / 2;
            if (lrows[i] <= 0 || lcols[i] <= 0) {
                return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid_build: level %d would be empty", i);
            }
        }
        slots[i] = L.take<uint8_t>(i > 0 || !image_on_device ? (size_t)lrows[i] * lcols[i] : 0);  // (level 0 of a device image stays the caller's)
    }
    if (!L.ok()) {
        return ftk_layout_refused(ctx);
    }
    const size_t total = L.bytes();
    ftk_pyramid *pyr = nullptr;
    int rc = make_pyramid(ctx, &pyr);
    if (rc != FTK_OK) {
        return rc;
    }
    hipError_t e = pyr->owned.reserve(ctx->stream, total, 0, 1);  // (nothing when level 0 is the caller's and there is no other)
    if (e != hipSuccess) {
        delete pyr;
        return ftk_fail(ctx, FTK_E_OUT_OF_MEMORY, "pyramid_build: device allocation of %zu bytes failed: %s", total, hipGetErrorString(e));
    }
    uint8_t *owned = pyr->owned.as<uint8_t>();
    pyr->n_levels = n_levels;
    // A host image goes through a pinned staging slot: the CPU copies it there (the caller's buffer is free on return), the
    // pyramid launch reads the slot over PCIe and keeps level 0 — no staged hipMemcpy of pageable memory, no stream
    // synchronisation (CreateImagePyramid x 2 sits inside the reference's timed region, test_optical_flow.cpp:69-73: 57 us per
    // build before).  One-level pyramids keep the copy.
    ftk_context::ImageStage *stage = nullptr;
    if (!image_on_device && n_levels >= 2) {
        rc = ftk_acquire_image_stage(ctx, (size_t)rows * cols, &stage);
        if (rc != FTK_OK) {
            ftk_pyramid_destroy(pyr);
            return rc;
        }
    }
    if (image_on_device) {
        pyr->levels[0].data = image;
    } else {
        if (stage) {
            memcpy(stage->host.get(), image, (size_t)rows * cols);
        } else {
            e = hipMemcpyAsync(owned, image, (size_t)rows * cols, hipMemcpyHostToDevice, ctx->stream);
        }
        pyr->levels[0].data = owned;
    }
    pyr->levels[0].rows = rows;
    pyr->levels[0].cols = cols;
    uint8_t *level_ptr[FTK_MAX_LEVELS] = {nullptr};
    for (int i = 1; i < n_levels; ++i) {
        level_ptr[i] = slots[i].in(owned);
        pyr->levels[i].data = level_ptr[i];
        pyr->levels[i].rows = lrows[i];
        pyr->levels[i].cols = lcols[i];
    }
    if (e == hipSuccess) {
        if (stage) {
            e = ftk::pyramid_build_levels_launch(stage->device_view, rows, cols, level_ptr, n_levels, ctx->stream, owned);
            if (e == hipSuccess) {
                e = hipEventRecord(stage->done, ctx->stream);
                stage->busy = e == hipSuccess;
            }
        } else {
            e = ftk::pyramid_build_levels_launch(pyr->levels[0].data, rows, cols, level_ptr, n_levels, ctx->stream);  // one launch for all levels
        }
    }
    if (e == hipSuccess && !image_on_device && !stage) {
        e = hipStreamSynchronize(ctx->stream);  // host image may be released by the caller
    }
    if (e != hipSuccess) {
        ftk_pyramid_destroy(pyr);
        return ftk_fail(ctx, FTK_E_HIP, "pyramid_build: %s", hipGetErrorString(e));
    }
    *out = pyr;
    return FTK_OK;
}

int ftk_pyramid_update(ftk_context *ctx, ftk_pyramid *pyr, const uint8_t *image, int image_location) {
    FTK_TRACE_SCOPE("ftk_pyramid_update");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "pyramid_update: null context");
    }
    FTK_LOCK(ctx);
    if (!pyr || !image || image_location < FTK_IMAGE_HOST || image_location > FTK_IMAGE_HOST_ASYNC) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid_update: null pyramid / image or unknown image location %d", image_location);
    }
    if (pyr->device != ctx->device) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid_update: the pyramid lives on another device");
    }
    uint8_t *owned = pyr->owned.as<uint8_t>();
    if (!owned || pyr->levels[0].data != owned) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "pyramid_update: only pyramids that own their level 0 (ftk_pyramid_upload, ftk_pyramid_build of a host image) can be refilled");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t *level_ptr[FTK_MAX_LEVELS] = {nullptr};
    bool halves = true;  // every level is the floor-half of the one above it (true for every pyramid this library builds)
    for (int i = 1; i < pyr->n_levels; ++i) {
        level_ptr[i] = const_cast<uint8_t *>(pyr->levels[i].data);
        halves = halves && pyr->levels[i].rows == pyr->levels[i - 1].rows / 2 && pyr->levels[i].cols == pyr->levels[i - 1].cols / 2;
    }
    if (!halves) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "pyramid_update: the levels of this pyramid are not successive halves (uploaded with another geometry)");
    }
    // A frame in PINNED host memory (FTK_IMAGE_HOST_ASYNC) is read by the pyramid launch itself when the device can address it:
    // the copy engine takes ~20 us per 300 KB frame, the kernel's own PCIe read a third of that, and a launch gap goes with it.
    // Pageable or unmapped memory takes the copy.
    const uint8_t *direct_src = nullptr;
    if (image_location == FTK_IMAGE_HOST_ASYNC && pyr->n_levels >= 2) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, image) == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer != nullptr) {
            direct_src = static_cast<const uint8_t *>(attr.devicePointer);
        } else {
            (void)hipGetLastError();  // not an error of this call: the copy path below serves the pointer
        }
    }
    ftk_context::ImageStage *stage = nullptr;
    if (image_location == FTK_IMAGE_HOST && pyr->n_levels >= 2) {
        // a pageable frame: CPU copy into a pinned slot (the caller's buffer is free on return), read by the launch; no synchronisation
        const int rc = ftk_acquire_image_stage(ctx, (size_t)pyr->levels[0].rows * pyr->levels[0].cols, &stage);
        if (rc != FTK_OK) {
            return rc;
        }
    }
    if (stage != nullptr) {
        memcpy(stage->host.get(), image, (size_t)pyr->levels[0].rows * pyr->levels[0].cols);
        FTK_HIP(ctx, ftk::pyramid_build_levels_launch(stage->device_view, pyr->levels[0].rows, pyr->levels[0].cols, level_ptr, pyr->n_levels, ctx->stream, owned));
        FTK_HIP(ctx, hipEventRecord(stage->done, ctx->stream));
        stage->busy = true;
        return FTK_OK;
    }
    if (direct_src != nullptr) {
        FTK_HIP(ctx, ftk::pyramid_build_levels_launch(direct_src, pyr->levels[0].rows, pyr->levels[0].cols, level_ptr, pyr->n_levels, ctx->stream, owned));
    } else {
        const size_t bytes0 = (size_t)pyr->levels[0].rows * pyr->levels[0].cols;
        FTK_HIP(ctx, hipMemcpyAsync(owned, image, bytes0, image_location == FTK_IMAGE_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                    ctx->stream));
        FTK_HIP(ctx, ftk::pyramid_build_levels_launch(pyr->levels[0].data, pyr->levels[0].rows, pyr->levels[0].cols, level_ptr, pyr->n_levels, ctx->stream));
    }
    if (image_location == FTK_IMAGE_HOST) {
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller may release or rewrite the host image on return
    }
    return FTK_OK;
}

int ftk_pyramid_levels(const ftk_pyramid *pyr) { return pyr ? pyr->n_levels : 0; }

int ftk_pyramid_level(const ftk_pyramid *pyr, int32_t level, ftk_image *out) {
    if (!pyr || !out || level < 0 || level >= pyr->n_levels) {
        return FTK_E_INVALID_ARGUMENT;
    }
    out->data = pyr->levels[level].data;
    out->rows = pyr->levels[level].rows;
    out->cols = pyr->levels[level].cols;
    return FTK_OK;
}

int ftk_pyramid_download_level(ftk_context *ctx, const ftk_pyramid *pyr, int32_t level, uint8_t *host_out) {
    FTK_TRACE_SCOPE("ftk_pyramid_download_level");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "pyramid_download_level: null context");
    }
    FTK_LOCK(ctx);
    if (!pyr || !host_out || level < 0 || level >= pyr->n_levels) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid_download_level: bad arguments");
    }
    const size_t bytes = (size_t)pyr->levels[level].rows * pyr->levels[level].cols;
    FTK_HIP(ctx, hipMemcpyAsync(host_out, pyr->levels[level].data, bytes, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

void ftk_pyramid_destroy(ftk_pyramid *pyr) {
    FTK_TRACE_SCOPE("ftk_pyramid_destroy");
    if (!pyr) {
        return;
    }
    if (pyr->owned) {
        (void)hipSetDevice(pyr->device);
    }
    delete pyr;  // and the levels it owns
}

}  // extern "C"
