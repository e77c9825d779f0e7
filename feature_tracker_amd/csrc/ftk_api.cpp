// ftk_api.cpp — the C ABI of libftk_hip.so (declared in include/ftk.h), except the trackers' entry points (ftk_klt.cpp).
//
// Host-side plumbing only: argument validation, device buffers, stream ordering, launches.
// All numerics live in the kernels.  There is deliberately no CPU fallback: if HIP is not
// usable every compute entry point fails with FTK_E_NO_DEVICE / FTK_E_HIP.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "ftk_device.h"
#include "ftk_internal.h"
#include "match_plan.h"

using ftk::DevImage;

thread_local std::string g_create_error;

int ftk_fail(ftk_context *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) {
        ctx->error = buf;
    } else {
        g_create_error = buf;
    }
    return code;
}

int ftk_ensure_scratch(ftk_context *ctx, size_t bytes) {
    if (bytes <= ctx->scratch_bytes) {
        return FTK_OK;
    }
    if (ctx->scratch) {
        FTK_HIP(ctx, hipFree(ctx->scratch));
        ctx->scratch = nullptr;
        ctx->scratch_bytes = 0;
    }
    const size_t want = ftk_align_up(bytes + bytes / 2, 4096);
    FTK_HIP(ctx, hipMalloc(&ctx->scratch, want));
    ctx->scratch_bytes = want;
    return FTK_OK;
}

int ftk_ensure_pinned(ftk_context *ctx, size_t bytes) {
    if (bytes <= ctx->pinned_bytes) {
        return FTK_OK;
    }
    if (ctx->pinned) {
        FTK_HIP(ctx, hipHostFree(ctx->pinned));
        ctx->pinned = nullptr;
        ctx->pinned_bytes = 0;
    }
    const size_t want = ftk_align_up(bytes + bytes / 2, 4096);
    // Coarse-grained (non-coherent) host memory: cacheable in the device's L2, coherent at kernel boundaries — which is all the
    // host-buffer entry points need (the host writes the block before the launch and reads it after the synchronisation).  The 2 000
    // workgroups of a zero-copy tracker call then share 64-byte lines instead of each crossing PCIe for its own 17 bytes, and their
    // results leave the chip as whole lines when the kernel ends: same box, 2 000-feature call 68.1 / 71.2 -> 66.2 / 65.6 us, small
    // calls unchanged (round 5).
    FTK_HIP(ctx, hipHostMalloc(&ctx->pinned, want, hipHostMallocNonCoherent));
    ctx->pinned_bytes = want;
    return FTK_OK;
}

namespace {

size_t align_up(size_t x, size_t a) { return ftk_align_up(x, a); }

// The next image-staging slot, free and at least `bytes` large (ftk_internal.h ImageStage); *out stays null when the device cannot
// address pinned host memory (the callers then take their copy paths).
int acquire_image_stage(ftk_context *ctx, size_t bytes, ftk_context::ImageStage **out) {
    *out = nullptr;
    ftk_context::ImageStage &st = ctx->image_stage[ctx->image_stage_next];
    if (st.busy) {
        FTK_HIP(ctx, hipEventSynchronize(st.done));  // normally long past: two frames per tracker call
        st.busy = false;
    }
    if (st.bytes < bytes) {
        if (st.host) {
            FTK_HIP(ctx, hipHostFree(st.host));
            st.host = nullptr;
            st.bytes = 0;
        }
        const size_t want = align_up(bytes, 1u << 20);
        void *h = nullptr, *d = nullptr;
        FTK_HIP(ctx, hipHostMalloc(&h, want, hipHostMallocDefault));
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess || d == nullptr) {
            (void)hipGetLastError();
            (void)hipHostFree(h);
            return FTK_OK;  // *out == nullptr
        }
        st.host = static_cast<uint8_t *>(h);
        st.device_view = static_cast<const uint8_t *>(d);
        st.bytes = want;
    }
    if (!st.done) {
        FTK_HIP(ctx, hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    }
    ctx->image_stage_next ^= 1;
    *out = &st;
    return FTK_OK;
}

int ensure_match_keys(ftk_context *ctx, size_t count) {
    if (count <= ctx->match_keys_count) {
        return FTK_OK;
    }
    if (ctx->match_keys) {
        FTK_HIP(ctx, hipFree(ctx->match_keys));
        ctx->match_keys = nullptr;
        ctx->match_keys_count = 0;
    }
    FTK_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->match_keys), sizeof(unsigned long long) * count));
    // all-ones = "no match yet"; the epilogue kernel restores this state after every call
    FTK_HIP(ctx, hipMemsetAsync(ctx->match_keys, 0xFF, sizeof(unsigned long long) * count, ctx->stream));
    ctx->match_keys_count = count;
    return FTK_OK;
}

int ensure_match_boxes(ftk_context *ctx, size_t count) {
    if (count <= ctx->match_boxes_count) {
        return FTK_OK;
    }
    if (ctx->match_boxes) {
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        FTK_HIP(ctx, hipFree(ctx->match_boxes));
        ctx->match_boxes = nullptr;
        ctx->match_boxes_count = 0;
    }
    FTK_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->match_boxes), sizeof(float) * 4 * count));
    ctx->match_boxes_count = count;
    return FTK_OK;
}

}  // namespace

// Grows a context-owned device buffer (stream-synchronising first: earlier launches may still read the old one).
int ftk_ensure_device_buffer(ftk_context *ctx, void **buf, size_t *have, size_t bytes) {
    if (bytes <= *have) {
        return FTK_OK;
    }
    if (*buf) {
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        FTK_HIP(ctx, hipFree(*buf));
        *buf = nullptr;
        *have = 0;
    }
    const size_t want = align_up(bytes + bytes / 4, 4096);
    FTK_HIP(ctx, hipMalloc(buf, want));
    *have = want;
    return FTK_OK;
}

namespace {

int ensure_device_buffer(ftk_context *ctx, void **buf, size_t *have, size_t bytes) { return ftk_ensure_device_buffer(ctx, buf, have, bytes); }

int make_pyramid(ftk_context *ctx, ftk_pyramid **out) {
    if (!ctx || !out) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid: null context or output");
    }
    ftk_pyramid *pyr = new (std::nothrow) ftk_pyramid();
    if (!pyr) {
        return fail(ctx, FTK_E_OUT_OF_MEMORY, "pyramid: host allocation failed");
    }
    pyr->device = ctx->device;
    *out = pyr;
    return FTK_OK;
}

// The trackers index a level with 32-bit pixel offsets formed on the 24-bit multiplier (klt_common.h px()).
bool level_addressable(int32_t rows, int32_t cols) { return rows < (1 << 24) && cols < (1 << 24) && (long long)rows * cols < (1ll << 32); }

int check_levels(ftk_context *ctx, const ftk_image *levels, int32_t n_levels) {
    if (!levels || n_levels < 1 || n_levels > FTK_MAX_LEVELS) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid: n_levels %d outside [1, %d]", n_levels, FTK_MAX_LEVELS);
    }
    for (int i = 0; i < n_levels; ++i) {
        if (!levels[i].data || levels[i].rows <= 0 || levels[i].cols <= 0) {
            return fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid: level %d is empty", i);
        }
        if (!level_addressable(levels[i].rows, levels[i].cols)) {
            return fail(ctx, FTK_E_UNSUPPORTED, "pyramid: level %d (%d x %d) exceeds 2^24 on a side or 2^32 pixels", i, levels[i].rows, levels[i].cols);
        }
    }
    return FTK_OK;
}

}  // namespace

extern "C" {

int ftk_abi_version(void) { return FTK_ABI_VERSION; }

int ftk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        return 0;
    }
    return n;
}

int ftk_context_create(int device, void *stream, ftk_context **out) {
    FTK_TRACE_SCOPE("ftk_context_create");
    if (!out) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "context: null output pointer");
    }
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        return fail(nullptr, FTK_E_NO_DEVICE, "context: no HIP device available (%s); this library has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    }
    if (device < 0) {
        FTK_HIP(nullptr, hipGetDevice(&device));
    }
    if (device >= count) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "context: device %d out of range (have %d)", device, count);
    }
    FTK_HIP(nullptr, hipSetDevice(device));
    ftk_context *ctx = new (std::nothrow) ftk_context();
    if (!ctx) {
        return fail(nullptr, FTK_E_OUT_OF_MEMORY, "context: host allocation failed");
    }
    ctx->device = device;
    if (stream) {
        ctx->stream = reinterpret_cast<hipStream_t>(stream);
        ctx->owns_stream = false;
    } else {
        hipError_t se = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (se != hipSuccess) {
            delete ctx;
            return fail(nullptr, FTK_E_HIP, "context: hipStreamCreate failed: %s", hipGetErrorString(se));
        }
        ctx->owns_stream = true;
    }
    ctx->env.read();
    if (const char *env = FTK_ENV(ctx, reduction)) {  // experiment switch: contexts start in the throughput mode ("tree"); default exact
        ctx->reduction = (strcmp(env, "tree") == 0) ? FTK_REDUCTION_TREE : FTK_REDUCTION_EXACT;
    }
    *out = ctx;
    return FTK_OK;
}

void ftk_context_destroy(ftk_context *ctx) {
    if (!ctx) {
        return;
    }
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->scratch) {
        (void)hipFree(ctx->scratch);
    }
    if (ctx->match_boxes) {
        (void)hipFree(ctx->match_boxes);
    }
    if (ctx->match_keys) {
        (void)hipFree(ctx->match_keys);
    }
    if (ctx->nn_keys) {
        (void)hipFree(ctx->nn_keys);
    }
    if (ctx->cosine_ws) {
        (void)hipFree(ctx->cosine_ws);
    }
    if (ctx->direct_table) {
        (void)hipFree(ctx->direct_table);
    }
    if (ctx->direct_feat) {
        (void)hipFree(ctx->direct_feat);
    }
    for (int k = 0; k < 2; ++k) {
        if (ctx->sched_iters[k]) {
            (void)hipFree(ctx->sched_iters[k]);
            (void)hipFree(ctx->sched_order[k]);
        }
    }
    if (ctx->klt_spill) {
        (void)hipFree(ctx->klt_spill);
    }
    if (ctx->direct_spread) {
        (void)hipFree(ctx->direct_spread);
    }
    if (ctx->match_pad) {
        (void)hipFree(ctx->match_pad);
    }
    if (ctx->tail_host) {
        (void)hipHostFree(ctx->tail_host);
    }
    if (ctx->tail_dev) {
        (void)hipFree(ctx->tail_dev);
    }
    if (ctx->sched_grid) {
        (void)hipFree(ctx->sched_grid);
    }
    if (ctx->sched_pred) {
        (void)hipFree(ctx->sched_pred);
    }
    if (ctx->sched_claim) {
        (void)hipFree(ctx->sched_claim);
    }
    for (auto &st : ctx->image_stage) {
        if (st.done) {
            (void)hipEventDestroy(st.done);
        }
        if (st.host) {
            (void)hipHostFree(st.host);
        }
    }
    if (ctx->pinned) {
        (void)hipHostFree(ctx->pinned);
    }
    if (ctx->brief_pattern) {
        (void)hipFree(ctx->brief_pattern);
    }
    if (ctx->dense_ws) {
        (void)hipFree(ctx->dense_ws);
    }
    if (ctx->dense_weights) {
        (void)hipFree(ctx->dense_weights);
    }
    if (ctx->owns_stream) {
        (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}

const char *ftk_last_error(const ftk_context *ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int ftk_synchronize(ftk_context *ctx) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "synchronize: null context");
    }
    FTK_LOCK(ctx);
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

static int ensure_brief_pattern(ftk_context *ctx, int32_t n_bits, int32_t half);

int ftk_context_refresh_env(ftk_context *ctx) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "context_refresh_env: null context");
    }
    FTK_LOCK(ctx);
    ctx->env.read();
    return FTK_OK;
}

int ftk_set_reduction_mode(ftk_context *ctx, int mode) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "set_reduction_mode: null context");
    }
    FTK_LOCK(ctx);
    if (mode != FTK_REDUCTION_EXACT && mode != FTK_REDUCTION_TREE) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "set_reduction_mode: unknown mode %d", mode);
    }
    ctx->reduction = mode;
    return FTK_OK;
}

int ftk_warmup(ftk_context *ctx, unsigned what) {
    FTK_TRACE_SCOPE("ftk_warmup");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "warmup: null context");
    }
    FTK_LOCK(ctx);
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    if (what & FTK_WARM_KLT) {
        FTK_HIP(ctx, ftk::klt_warm(ctx->stream));
        FTK_HIP(ctx, ftk::klt_basic_warm(ctx->stream));
        FTK_HIP(ctx, ftk::klt_fast_warm(ctx->stream));
        FTK_HIP(ctx, ftk::pyramid_warm(ctx->stream));
        // the staging blocks of the host-buffer entry points, at the size a few thousand features need ...
        // ... and what the upload of one 1080p pyramid stages (ftk_pyramid_upload gathers the levels in the pinned block)
        int rc = ftk_ensure_scratch(ctx, 4u << 20);
        if (rc == FTK_OK) {
            rc = ftk_ensure_pinned(ctx, 4u << 20);
        }
        // ... and the two pinned slots host images pass through on their way into a pyramid (1 MB each: up to 1024 x 1024)
        for (int k = 0; k < 2 && rc == FTK_OK; ++k) {
            ftk_context::ImageStage *stage = nullptr;
            rc = acquire_image_stage(ctx, 1u << 20, &stage);
        }
        if (rc != FTK_OK) {
            return rc;
        }
    }
    if (what & FTK_WARM_HAMMING) {
        FTK_HIP(ctx, ftk::matcher_warm(ctx->stream));
        FTK_HIP(ctx, ftk::feature_warm(ctx->stream));  // BRIEF descriptors sit in front of the matcher
        int rc = ensure_match_keys(ctx, 4096);
        if (rc == FTK_OK) {
            rc = ftk_ensure_scratch(ctx, 4u << 20);
        }
        if (rc == FTK_OK) {
            rc = ftk_ensure_pinned(ctx, 4u << 20);
        }
        if (rc == FTK_OK) {
            rc = ensure_brief_pattern(ctx, 256, 8);  // kLength / kHalfPatchSize of the reference's caller (test_descriptor_matcher_brief.cpp:71-72)
        }
        if (rc != FTK_OK) {
            return rc;
        }
    }
    if (what & FTK_WARM_COSINE) {
        FTK_HIP(ctx, ftk::cosine_warm(ctx->stream));
        FTK_HIP(ctx, ftk::nn_match_warm(ctx->stream));  // LightGlue's post-processing sits behind the same float descriptors
    }
    if (what & FTK_WARM_DIRECT) {
        FTK_HIP(ctx, ftk::direct_warm(ctx->stream));
        FTK_HIP(ctx, ftk::pyramid_warm(ctx->stream));
    }
    if (what & FTK_WARM_FEATURES) {
        FTK_HIP(ctx, ftk::feature_warm(ctx->stream));
    }
    // ... and one REAL launch of every kernel a default-configured object of the family would launch first: besides its code
    // object a kernel's very first launch costs 0.2 - 1 ms of its own (measured: the first TrackFeatures of a process 0.41 / 1.33 ms
    // on two boxes against 0.17 ms for the second tracker).  A 64 x 64 all-zero image, one feature / descriptor / point; results
    // are discarded, failures ignored (warm-up is best effort and must not leave an error behind).
    {
        const std::string saved_error = ctx->error;
        uint8_t *dummy = nullptr;
        constexpr size_t kImg = 64 * 64, kOff = 8192;  // image | feature block | descriptors
        if (hipMalloc(reinterpret_cast<void **>(&dummy), kOff + 8192) == hipSuccess &&
            hipMemsetAsync(dummy, 0, kOff + 8192, ctx->stream) == hipSuccess) {
            static_assert(kImg <= kOff, "dummy image fits in front of the feature block");
            ftk_image level = {dummy, 64, 64};
            ftk_pyramid *pyr = nullptr;
            float *d_uv = reinterpret_cast<float *>(dummy + kOff);          // ref (u, v) = (0, 0): never dereferenced out of range
            float *d_cur = d_uv + 2, *d_out = d_uv + 4;
            uint8_t *d_st = dummy + kOff + 64, *d_sto = dummy + kOff + 128;
            uint32_t *d_desc_ref = reinterpret_cast<uint32_t *>(dummy + kOff + 256), *d_desc_cur = d_desc_ref + 16;
            int32_t *d_idx = reinterpret_cast<int32_t *>(dummy + kOff + 512);
            float *d_fref = reinterpret_cast<float *>(dummy + kOff + 1024), *d_fcur = d_fref + 256;
            if (ftk_pyramid_wrap_device(ctx, &level, 1, &pyr) == FTK_OK) {
                if (what & FTK_WARM_KLT) {
                    ftk_klt_options opt;
                    ftk_default_klt_options(&opt);
                    for (int model = FTK_MODEL_BASIC; model <= FTK_MODEL_LSSD; ++model) {
                        for (int method = FTK_METHOD_INVERSE; method <= FTK_METHOD_FAST; ++method) {
                            opt.method = method;
                            (void)ftk_klt_track_device(ctx, model, &opt, pyr, pyr, d_uv, d_cur, d_out, d_st, d_sto, 1, nullptr, 0, 0, nullptr);
                        }
                    }
                }
                if (what & (FTK_WARM_HAMMING | FTK_WARM_FEATURES)) {
                    (void)ftk_brief_compute_device(ctx, pyr, 0, d_uv, 1, 256, 8, d_desc_ref);
                }
                if (what & FTK_WARM_FEATURES) {
                    float corner[2];
                    int32_t found = 0;
                    (void)ftk_harris_detect(ctx, pyr, 0, 1, 25, 40.0f, corner, &found);
                }
                if (what & FTK_WARM_DIRECT) {
                    ftk_direct_options dopt;
                    ftk_default_direct_options(&dopt);
                    const float K[4] = {64.0f, 64.0f, 32.0f, 32.0f}, point[3] = {0.0f, 0.0f, 1.0f}, ruv[2] = {32.0f, 32.0f};
                    float cuv[2] = {32.0f, 32.0f}, q[4] = {1.0f, 0.0f, 0.0f, 0.0f}, t[3] = {0.0f, 0.0f, 0.0f};
                    uint8_t st = 0;
                    (void)ftk_direct_track(ctx, &dopt, pyr, pyr, K, point, ruv, cuv, 1, q, t, &st, 0, nullptr);
                }
                ftk_pyramid_destroy(pyr);
            }
            if (what & FTK_WARM_HAMMING) {
                (void)ftk_hamming_match_device(ctx, d_desc_ref, 1, d_desc_cur, 1, 8, 256, 60.0f, nullptr, nullptr, 40, 40, d_idx, nullptr);
                (void)ftk_hamming_match_device(ctx, d_desc_ref, 1, d_desc_cur, 1, 8, 256, 60.0f, d_uv, d_cur, 40, 40, d_idx, nullptr);
            }
            if (what & FTK_WARM_COSINE) {
                for (int dim : {256, 128}) {
                    (void)ftk_cosine_match_device(ctx, d_fref, 1, d_fcur, 1, dim, 0.5f, nullptr, nullptr, 40, 40, d_idx);
                    (void)ftk_cosine_match_device(ctx, d_fref, 1, d_fcur, 1, dim, 0.5f, d_uv, d_cur, 40, 40, d_idx);
                }
            }
            (void)hipStreamSynchronize(ctx->stream);
        }
        if (dummy) {
            (void)hipFree(dummy);
        }
        ctx->error = saved_error;
    }
    if (ctx->pinned && ctx->scratch) {
        // first copies in both directions between the staging blocks (the copy path's first use is not free either)
        // (an image-sized one: copies beyond a few KB take another path in the runtime than small ones, and the first 361 KB
        // upload of a process was measured at 5.8 - 7.9 ms)
        const size_t probe = ctx->pinned_bytes < ctx->scratch_bytes ? ctx->pinned_bytes : ctx->scratch_bytes;
        FTK_HIP(ctx, hipMemcpyAsync(ctx->scratch, ctx->pinned, probe, hipMemcpyHostToDevice, ctx->stream));
        FTK_HIP(ctx, hipMemcpyAsync(ctx->pinned, ctx->scratch, probe, hipMemcpyDeviceToHost, ctx->stream));
        void *tmp = nullptr;  // and one image-sized allocation: what every ftk_pyramid_upload / ftk_pyramid_build makes
        if (hipMalloc(&tmp, 4u << 20) == hipSuccess) {
            (void)hipFree(tmp);
        }
    }
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

/* ---- pyramids ------------------------------------------------------------------------------ */

int ftk_pyramid_upload(ftk_context *ctx, const ftk_image *host_levels, int32_t n_levels, ftk_pyramid **out) {
    FTK_TRACE_SCOPE("ftk_pyramid_upload");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "pyramid_upload: null context");
    }
    FTK_LOCK(ctx);
    int rc = check_levels(ctx, host_levels, n_levels);
    if (rc != FTK_OK) {
        return rc;
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    size_t offsets[FTK_MAX_LEVELS];
    size_t total = 0;
    for (int i = 0; i < n_levels; ++i) {
        offsets[i] = total;
        total += align_up((size_t)host_levels[i].rows * host_levels[i].cols, 256);
    }
    ftk_pyramid *pyr = nullptr;
    rc = make_pyramid(ctx, &pyr);
    if (rc != FTK_OK) {
        return rc;
    }
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&pyr->owned), total);
    if (e != hipSuccess) {
        delete pyr;
        return fail(ctx, FTK_E_OUT_OF_MEMORY, "pyramid_upload: hipMalloc(%zu) failed: %s", total, hipGetErrorString(e));
    }
    pyr->n_levels = n_levels;
    // gather the levels in pinned staging, then ONE H2D copy of the whole pyramid
    if (ftk_ensure_pinned(ctx, total) != FTK_OK) {
        ftk_pyramid_destroy(pyr);
        return FTK_E_OUT_OF_MEMORY;
    }
    uint8_t *staging = static_cast<uint8_t *>(ctx->pinned);
    for (int i = 0; i < n_levels; ++i) {
        const size_t bytes = (size_t)host_levels[i].rows * host_levels[i].cols;
        memcpy(staging + offsets[i], host_levels[i].data, bytes);
        pyr->levels[i].data = pyr->owned + offsets[i];
        pyr->levels[i].rows = host_levels[i].rows;
        pyr->levels[i].cols = host_levels[i].cols;
    }
    e = hipMemcpyAsync(pyr->owned, staging, total, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        e = hipStreamSynchronize(ctx->stream);  // staging and the caller's buffers are free again on return
    }
    if (e != hipSuccess) {
        ftk_pyramid_destroy(pyr);
        return fail(ctx, FTK_E_HIP, "pyramid_upload: copy failed: %s", hipGetErrorString(e));
    }
    *out = pyr;
    return FTK_OK;
}

int ftk_pyramid_wrap_device(ftk_context *ctx, const ftk_image *device_levels, int32_t n_levels, ftk_pyramid **out) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "pyramid_wrap_device: null context");
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
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "pyramid_build: null context");
    }
    FTK_LOCK(ctx);
    if (!image || rows <= 0 || cols <= 0 || n_levels < 1 || n_levels > FTK_MAX_LEVELS || !out) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid_build: bad image or level count");
    }
    if (!level_addressable(rows, cols)) {
        return fail(ctx, FTK_E_UNSUPPORTED, "pyramid_build: image %d x %d exceeds 2^24 on a side or 2^32 pixels", rows, cols);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    int32_t lrows[FTK_MAX_LEVELS], lcols[FTK_MAX_LEVELS];
    size_t offsets[FTK_MAX_LEVELS];
    size_t total = 0;
    lrows[0] = rows;
    lcols[0] = cols;
    for (int i = 0; i < n_levels; ++i) {
        if (i > 0) {
            lrows[i] = lrows[i - 1] / 2;
            lcols[i] = lcols[i - 1] / 2;
            if (lrows[i] <= 0 || lcols[i] <= 0) {
                return fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid_build: level %d would be empty", i);
            }
        }
        offsets[i] = total;
        if (i > 0 || !image_on_device) {
            total += align_up((size_t)lrows[i] * lcols[i], 256);
        }
    }
    ftk_pyramid *pyr = nullptr;
    int rc = make_pyramid(ctx, &pyr);
    if (rc != FTK_OK) {
        return rc;
    }
    if (total > 0) {
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&pyr->owned), total);
        if (e != hipSuccess) {
            delete pyr;
            return fail(ctx, FTK_E_OUT_OF_MEMORY, "pyramid_build: hipMalloc(%zu) failed: %s", total, hipGetErrorString(e));
        }
    }
    pyr->n_levels = n_levels;
    hipError_t e = hipSuccess;
    // A host image goes through a pinned staging slot: the CPU copies it there (the caller's buffer is free on return), the
    // pyramid launch reads the slot over PCIe and keeps level 0 — no staged hipMemcpy of pageable memory, no stream
    // synchronisation (CreateImagePyramid x 2 sits inside the reference's timed region, test_optical_flow.cpp:69-73: 57 us per
    // build before).  One-level pyramids keep the copy.
    ftk_context::ImageStage *stage = nullptr;
    if (!image_on_device && n_levels >= 2) {
        rc = acquire_image_stage(ctx, (size_t)rows * cols, &stage);
        if (rc != FTK_OK) {
            ftk_pyramid_destroy(pyr);
            return rc;
        }
    }
    if (image_on_device) {
        pyr->levels[0].data = image;
    } else {
        if (stage) {
            memcpy(stage->host, image, (size_t)rows * cols);
        } else {
            e = hipMemcpyAsync(pyr->owned, image, (size_t)rows * cols, hipMemcpyHostToDevice, ctx->stream);
        }
        pyr->levels[0].data = pyr->owned;
    }
    pyr->levels[0].rows = rows;
    pyr->levels[0].cols = cols;
    uint8_t *level_ptr[FTK_MAX_LEVELS] = {nullptr};
    for (int i = 1; i < n_levels; ++i) {
        level_ptr[i] = pyr->owned + offsets[i];
        pyr->levels[i].data = level_ptr[i];
        pyr->levels[i].rows = lrows[i];
        pyr->levels[i].cols = lcols[i];
    }
    if (e == hipSuccess) {
        if (stage) {
            e = ftk::pyramid_build_levels_launch(stage->device_view, rows, cols, level_ptr, n_levels, ctx->stream, pyr->owned);
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
        return fail(ctx, FTK_E_HIP, "pyramid_build: %s", hipGetErrorString(e));
    }
    *out = pyr;
    return FTK_OK;
}

int ftk_pyramid_update(ftk_context *ctx, ftk_pyramid *pyr, const uint8_t *image, int image_location) {
    FTK_TRACE_SCOPE("ftk_pyramid_update");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "pyramid_update: null context");
    }
    FTK_LOCK(ctx);
    if (!pyr || !image || image_location < FTK_IMAGE_HOST || image_location > FTK_IMAGE_HOST_ASYNC) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid_update: null pyramid / image or unknown image location %d", image_location);
    }
    if (pyr->device != ctx->device) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid_update: the pyramid lives on another device");
    }
    if (!pyr->owned || pyr->levels[0].data != pyr->owned) {
        return fail(ctx, FTK_E_UNSUPPORTED, "pyramid_update: only pyramids that own their level 0 (ftk_pyramid_upload, ftk_pyramid_build of a host image) can be refilled");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t *level_ptr[FTK_MAX_LEVELS] = {nullptr};
    bool halves = true;  // every level is the floor-half of the one above it (true for every pyramid this library builds)
    for (int i = 1; i < pyr->n_levels; ++i) {
        level_ptr[i] = const_cast<uint8_t *>(pyr->levels[i].data);
        halves = halves && pyr->levels[i].rows == pyr->levels[i - 1].rows / 2 && pyr->levels[i].cols == pyr->levels[i - 1].cols / 2;
    }
    if (!halves) {
        return fail(ctx, FTK_E_UNSUPPORTED, "pyramid_update: the levels of this pyramid are not successive halves (uploaded with another geometry)");
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
        const int rc = acquire_image_stage(ctx, (size_t)pyr->levels[0].rows * pyr->levels[0].cols, &stage);
        if (rc != FTK_OK) {
            return rc;
        }
    }
    if (stage != nullptr) {
        memcpy(stage->host, image, (size_t)pyr->levels[0].rows * pyr->levels[0].cols);
        FTK_HIP(ctx, ftk::pyramid_build_levels_launch(stage->device_view, pyr->levels[0].rows, pyr->levels[0].cols, level_ptr, pyr->n_levels, ctx->stream, pyr->owned));
        FTK_HIP(ctx, hipEventRecord(stage->done, ctx->stream));
        stage->busy = true;
        return FTK_OK;
    }
    if (direct_src != nullptr) {
        FTK_HIP(ctx, ftk::pyramid_build_levels_launch(direct_src, pyr->levels[0].rows, pyr->levels[0].cols, level_ptr, pyr->n_levels, ctx->stream, pyr->owned));
    } else {
        const size_t bytes0 = (size_t)pyr->levels[0].rows * pyr->levels[0].cols;
        FTK_HIP(ctx, hipMemcpyAsync(pyr->owned, image, bytes0, image_location == FTK_IMAGE_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
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
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "pyramid_download_level: null context");
    }
    FTK_LOCK(ctx);
    if (!pyr || !host_out || level < 0 || level >= pyr->n_levels) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "pyramid_download_level: bad arguments");
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
        (void)hipFree(pyr->owned);
    }
    delete pyr;
}

/* ---- BRIEF descriptors (producer of the matcher's input) ----------------------------------- */

static int ensure_brief_pattern(ftk_context *ctx, int32_t n_bits, int32_t half) {
    if (ctx->brief_pattern && ctx->brief_bits == n_bits && ctx->brief_half == half) {
        return FTK_OK;
    }
    if (ctx->brief_pattern) {
        FTK_HIP(ctx, hipFree(ctx->brief_pattern));
        ctx->brief_pattern = nullptr;
    }
    // LCG pattern: x <- 1664525 x + 1013904223 (seed 0x2545F491), offset = ((x >> 8) mod (2 half + 1)) - half
    std::vector<int8_t> pattern((size_t)4 * n_bits);
    uint32_t state = 0x2545F491u;
    const uint32_t span = (uint32_t)(2 * half + 1);
    for (auto &v : pattern) {
        state = state * 1664525u + 1013904223u;
        v = (int8_t)((int32_t)((state >> 8) % span) - half);
    }
    FTK_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->brief_pattern), pattern.size()));
    // through the pinned block on the context's stream: a pageable hipMemcpy on the null stream costs milliseconds the first time
    const int prc = ftk_ensure_pinned(ctx, pattern.size());
    if (prc != FTK_OK) {
        return prc;
    }
    memcpy(ctx->pinned, pattern.data(), pattern.size());
    FTK_HIP(ctx, hipMemcpyAsync(ctx->brief_pattern, ctx->pinned, pattern.size(), hipMemcpyHostToDevice, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the pinned block is reused by the caller right away
    ctx->brief_bits = n_bits;
    ctx->brief_half = half;
    return FTK_OK;
}

int ftk_brief_compute_device(ftk_context *ctx, const ftk_pyramid *image, int32_t level, const float *d_uv, int32_t n, int32_t n_bits,
                             int32_t half_patch, uint32_t *d_words) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "brief_compute_device: null context");
    }
    FTK_LOCK(ctx);
    if (!image || level < 0 || level >= image->n_levels || n < 0 || n_bits <= 0 || half_patch <= 0 || half_patch > 63) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "brief_compute_device: bad arguments (n %d, bits %d, half %d)", n, n_bits, half_patch);
    }
    if (n == 0) {
        return FTK_OK;
    }
    if (!d_uv || !d_words) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "brief_compute_device: null buffer");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_brief_pattern(ctx, n_bits, half_patch);
    if (rc != FTK_OK) {
        return rc;
    }
    ftk::BriefParams p;
    p.img = image->levels[level];
    p.uv = d_uv;
    p.words = d_words;
    p.pattern = ctx->brief_pattern;
    p.n = n;
    p.n_bits = n_bits;
    p.n_words = (n_bits + 31) / 32;
    p.half = half_patch;
    FTK_HIP(ctx, ftk::brief_launch(p, ctx->stream));
    return FTK_OK;
}

int ftk_brief_compute(ftk_context *ctx, const ftk_pyramid *image, int32_t level, const float *uv, int32_t n, int32_t n_bits,
                      int32_t half_patch, uint32_t *words) {
    FTK_TRACE_SCOPE("ftk_brief_compute");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "brief_compute: null context");
    }
    FTK_LOCK(ctx);
    if (n < 0 || n_bits <= 0) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "brief_compute: bad sizes");
    }
    if (n == 0) {
        return FTK_OK;
    }
    if (!uv || !words) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "brief_compute: null buffer");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_words = (size_t)(n_bits + 31) / 32;
    const size_t uv_bytes = align_up(sizeof(float) * 2 * (size_t)n, 256);
    const size_t w_bytes = align_up(sizeof(uint32_t) * n_words * (size_t)n, 256);
    int rc = ftk_ensure_scratch(ctx, uv_bytes + w_bytes);
    if (rc != FTK_OK) {
        return rc;
    }
    if (n_bits <= 0 || half_patch <= 0 || half_patch > 63) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "brief_compute: bad arguments (bits %d, half %d)", n_bits, half_patch);
    }
    rc = ensure_brief_pattern(ctx, n_bits, half_patch);  // before the pinned block is filled: it stages the pattern there
    if (rc == FTK_OK) {
        rc = ftk_ensure_pinned(ctx, uv_bytes + w_bytes);
    }
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *base = static_cast<uint8_t *>(ctx->scratch), *hbase = static_cast<uint8_t *>(ctx->pinned);
    float *d_uv = reinterpret_cast<float *>(base);
    uint32_t *d_words = reinterpret_cast<uint32_t *>(base + uv_bytes);
    memcpy(hbase, uv, sizeof(float) * 2 * (size_t)n);
    FTK_HIP(ctx, hipMemcpyAsync(d_uv, hbase, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    rc = ftk_brief_compute_device(ctx, image, level, d_uv, n, n_bits, half_patch, d_words);
    if (rc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    FTK_HIP(ctx, hipMemcpyAsync(hbase + uv_bytes, d_words, sizeof(uint32_t) * n_words * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(words, hbase + uv_bytes, sizeof(uint32_t) * n_words * (size_t)n);
    return FTK_OK;
}

/* ---- Harris corners (producer of the trackers' input) -------------------------------------- */

static int harris_run(ftk_context *ctx, const ftk_pyramid *image, int32_t level, int32_t min_distance, float min_response, float *response_out,
                      std::vector<unsigned long long> *survivors) {
    if (!image || level < 0 || level >= image->n_levels) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "harris: bad image / level");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const DevImage img = image->levels[level];
    const size_t px = (size_t)img.rows * img.cols;
    const size_t capacity = px;  // worst case (min_distance 1): every candidate is its own window maximum
    const size_t g_bytes = align_up(sizeof(short) * px, 256), f_bytes = align_up(sizeof(float) * px, 256);
    const size_t k_bytes = align_up(sizeof(unsigned long long) * px, 256), l_bytes = align_up(sizeof(unsigned long long) * capacity, 256);
    const int rc = ftk_ensure_scratch(ctx, 2 * g_bytes + f_bytes + 3 * k_bytes + l_bytes + 256);
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *base = static_cast<uint8_t *>(ctx->scratch);
    ftk::HarrisParams p;
    p.img = img;
    p.gx = reinterpret_cast<short *>(base);
    p.gy = reinterpret_cast<short *>(base + g_bytes);
    p.response = response_out ? reinterpret_cast<float *>(base + 2 * g_bytes) : nullptr;
    p.key = reinterpret_cast<unsigned long long *>(base + 2 * g_bytes + f_bytes);
    p.tmp = p.key + k_bytes / sizeof(unsigned long long);
    p.wmax = p.tmp + k_bytes / sizeof(unsigned long long);
    p.list = survivors ? p.wmax + k_bytes / sizeof(unsigned long long) : nullptr;
    p.count = reinterpret_cast<unsigned *>(base + 2 * g_bytes + f_bytes + 3 * k_bytes + l_bytes);
    p.capacity = (unsigned)capacity;
    p.min_distance = min_distance;
    p.min_response = min_response;
    FTK_HIP(ctx, ftk::harris_launch(p, ctx->stream));
    if (response_out) {
        FTK_HIP(ctx, hipMemcpyAsync(response_out, p.response, sizeof(float) * px, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (survivors) {
        unsigned count = 0;
        FTK_HIP(ctx, hipMemcpyAsync(&count, p.count, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (count > p.capacity) {
            return fail(ctx, FTK_E_UNSUPPORTED, "harris: %u survivors exceed the list capacity %u", count, p.capacity);
        }
        survivors->resize(count);
        if (count > 0) {
            FTK_HIP(ctx, hipMemcpyAsync(survivors->data(), p.list, sizeof(unsigned long long) * count, hipMemcpyDeviceToHost, ctx->stream));
            FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
    } else {
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return FTK_OK;
}

int ftk_harris_response(ftk_context *ctx, const ftk_pyramid *image, int32_t level, float *response) {
    FTK_TRACE_SCOPE("ftk_harris_response");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "harris_response: null context");
    }
    FTK_LOCK(ctx);
    if (!response) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "harris_response: null buffer");
    }
    return harris_run(ctx, image, level, 1, 0.0f, response, nullptr);
}

int ftk_harris_detect(ftk_context *ctx, const ftk_pyramid *image, int32_t level, int32_t max_count, int32_t min_distance, float min_response,
                      float *uv, int32_t *n_out) {
    FTK_TRACE_SCOPE("ftk_harris_detect");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "harris_detect: null context");
    }
    FTK_LOCK(ctx);
    if (!n_out || max_count < 0 || (max_count > 0 && !uv)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "harris_detect: bad output arguments");
    }
    *n_out = 0;
    if (!image || level < 0 || level >= image->n_levels) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "harris_detect: bad image / level");
    }
    const DevImage img = image->levels[level];
    if (max_count == 0 || img.rows < 23 || img.cols < 23) {
        return FTK_OK;
    }
    std::vector<unsigned long long> survivors;
    const int rc = harris_run(ctx, image, level, min_distance, min_response, nullptr, &survivors);
    if (rc != FTK_OK) {
        return rc;
    }
    // key order == (response descending, pixel index ascending): the final top-N selection is a sort of
    // a few thousand 64-bit keys on the host
    std::sort(survivors.begin(), survivors.end(), [](unsigned long long a, unsigned long long b) { return a > b; });
    const size_t n = survivors.size() < (size_t)max_count ? survivors.size() : (size_t)max_count;
    for (size_t i = 0; i < n; ++i) {
        const unsigned idx = 0xFFFFFFFFu - (unsigned)(survivors[i] & 0xFFFFFFFFull);
        uv[2 * i] = (float)(idx % (unsigned)img.cols);
        uv[2 * i + 1] = (float)(idx / (unsigned)img.cols);
    }
    *n_out = (int32_t)n;
    return FTK_OK;
}

/* ---- matcher ------------------------------------------------------------------------------- */

extern "C++" {
namespace {

int env_int(const char *v) { return v ? atoi(v) : ftk::kPlanNotSet; }

// Zero-pads the n_words-wide descriptors to `dev_words` words in a context-owned copy (equal pad bits in both sets: same distances).
int pad_descriptors(ftk_context *ctx, const uint32_t **ref, int32_t n_ref, const uint32_t **cur, int32_t n_cur, int32_t n_words, int32_t dev_words) {
    const size_t ref_bytes = align_up(sizeof(uint32_t) * (size_t)n_ref * dev_words, 256);
    const size_t cur_bytes = align_up(sizeof(uint32_t) * (size_t)n_cur * dev_words, 256);
    const int rc = ensure_device_buffer(ctx, &ctx->match_pad, &ctx->match_pad_bytes, ref_bytes + cur_bytes);
    if (rc != FTK_OK) {
        return rc;
    }
    uint32_t *pad_ref = static_cast<uint32_t *>(ctx->match_pad);
    uint32_t *pad_cur = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(ctx->match_pad) + ref_bytes);
    FTK_HIP(ctx, hipMemsetAsync(ctx->match_pad, 0, ref_bytes + cur_bytes, ctx->stream));
    FTK_HIP(ctx, hipMemcpy2DAsync(pad_ref, sizeof(uint32_t) * dev_words, *ref, sizeof(uint32_t) * n_words, sizeof(uint32_t) * n_words, (size_t)n_ref,
                                  hipMemcpyDeviceToDevice, ctx->stream));
    FTK_HIP(ctx, hipMemcpy2DAsync(pad_cur, sizeof(uint32_t) * dev_words, *cur, sizeof(uint32_t) * n_words, sizeof(uint32_t) * n_words, (size_t)n_cur,
                                  hipMemcpyDeviceToDevice, ctx->stream));
    *ref = pad_ref;
    *cur = pad_cur;
    return FTK_OK;
}

// The host-buffer matchers: [ref | cur | pred | cur_uv | index] gathered in the context's pinned block, laid out like the device
// scratch, and sent with ONE H2D (pageable hipMemcpyAsync calls are staged one by one by the runtime, ~10 us each; the reference's
// callers time these calls); `run` launches the device entry on the scratch copies, then the indices come back.  Descriptor rows of
// `row_bytes` are zero-padded to `dev_row_bytes` (pad bits equal in both sets: distance unchanged).
template <class Run>
int run_staged_match(ftk_context *ctx, const void *ref, int32_t n_ref, const void *cur, int32_t n_cur, size_t row_bytes, size_t dev_row_bytes,
                     const float *pred_uv, const float *cur_uv, int32_t *index_pairs, Run run) {
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ref_bytes = align_up(dev_row_bytes * (size_t)n_ref, 256);
    const size_t cur_bytes = align_up(dev_row_bytes * (size_t)n_cur, 256);
    const size_t pred_bytes = pred_uv ? align_up(sizeof(float) * 2 * (size_t)n_ref, 256) : 0;
    const size_t cuv_bytes = pred_uv ? align_up(sizeof(float) * 2 * (size_t)n_cur, 256) : 0;
    const size_t idx_at = ref_bytes + cur_bytes + pred_bytes + cuv_bytes, in_bytes = idx_at + align_up(sizeof(int32_t) * (size_t)n_ref, 256);
    int rc = ftk_ensure_scratch(ctx, in_bytes);
    rc = rc == FTK_OK ? ftk_ensure_pinned(ctx, in_bytes) : rc;
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *base = static_cast<uint8_t *>(ctx->scratch), *hbase = static_cast<uint8_t *>(ctx->pinned);
    if (dev_row_bytes == row_bytes) {
        memcpy(hbase, ref, row_bytes * (size_t)n_ref);
        memcpy(hbase + ref_bytes, cur, row_bytes * (size_t)n_cur);
    } else {
        memset(hbase, 0, ref_bytes + cur_bytes);
        for (int32_t i = 0; i < n_ref; ++i) {
            memcpy(hbase + dev_row_bytes * (size_t)i, static_cast<const uint8_t *>(ref) + row_bytes * (size_t)i, row_bytes);
        }
        for (int32_t i = 0; i < n_cur; ++i) {
            memcpy(hbase + ref_bytes + dev_row_bytes * (size_t)i, static_cast<const uint8_t *>(cur) + row_bytes * (size_t)i, row_bytes);
        }
    }
    if (pred_uv) {
        memcpy(hbase + ref_bytes + cur_bytes, pred_uv, sizeof(float) * 2 * (size_t)n_ref);
        memcpy(hbase + ref_bytes + cur_bytes + pred_bytes, cur_uv, sizeof(float) * 2 * (size_t)n_cur);
    }
    memcpy(hbase + idx_at, index_pairs, sizeof(int32_t) * (size_t)n_ref);
    FTK_HIP(ctx, hipMemcpyAsync(base, hbase, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    int32_t *d_idx = reinterpret_cast<int32_t *>(base + idx_at);
    rc = run(base, base + ref_bytes, pred_uv ? reinterpret_cast<float *>(base + ref_bytes + cur_bytes) : nullptr,
             pred_uv ? reinterpret_cast<float *>(base + ref_bytes + cur_bytes + pred_bytes) : nullptr, d_idx);
    if (rc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    FTK_HIP(ctx, hipMemcpyAsync(hbase + idx_at, d_idx, sizeof(int32_t) * (size_t)n_ref, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(index_pairs, hbase + idx_at, sizeof(int32_t) * (size_t)n_ref);
    return FTK_OK;
}

}  // namespace
}  // extern "C++"

int ftk_hamming_match_device(ftk_context *ctx, const uint32_t *d_ref_words, int32_t n_ref, const uint32_t *d_cur_words, int32_t n_cur,
                             int32_t n_words, int32_t n_bits, float max_distance, const float *d_pred_uv, const float *d_cur_uv,
                             int32_t max_col_distance, int32_t max_row_distance, int32_t *d_index_pairs, uint64_t *d_workspace) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "hamming_match_device: null context");
    }
    FTK_LOCK(ctx);
    if (n_ref < 0 || n_cur < 0 || n_bits < 0) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "hamming_match_device: negative size");
    }
    if (n_ref == 0 || n_cur == 0) {
        return FTK_OK;
    }
    if (n_words < 1) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "hamming_match_device: n_words %d < 1", n_words);
    }
    if (n_bits > 32 * n_words) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "hamming_match_device: n_bits %d exceeds %d words", n_bits, n_words);
    }
    if (!d_ref_words || !d_cur_words || !d_index_pairs || (d_pred_uv && !d_cur_uv)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "hamming_match_device: null buffer");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const char *kernel = FTK_ENV(ctx, match_kernel);
    const ftk::HammingPlan plan = ftk::hamming_plan({n_ref, n_cur, n_words, n_bits, d_pred_uv != nullptr, d_workspace != nullptr, env_int(FTK_ENV(ctx, match_small)),
                                                     kernel ? (strcmp(kernel, "mfma") == 0 ? 1 : 0) : ftk::kPlanNotSet});
    int rc = plan.dev_words != n_words ? pad_descriptors(ctx, &d_ref_words, n_ref, &d_cur_words, n_cur, n_words, plan.dev_words) : FTK_OK;
    rc = rc == FTK_OK && plan.keys_clean ? ensure_match_keys(ctx, (size_t)n_ref) : rc;  // (the context's keys hold "no match")
    rc = rc == FTK_OK && plan.n_boxes > 0 ? ensure_match_boxes(ctx, plan.n_boxes) : rc;
    if (rc != FTK_OK) {
        return rc;
    }
    unsigned long long *keys = plan.keys_clean ? ctx->match_keys : reinterpret_cast<unsigned long long *>(d_workspace);
    const ftk::MatchParams p = {d_ref_words, d_cur_words, d_pred_uv, d_cur_uv, d_index_pairs, keys, n_ref, n_cur, plan.dev_words, n_bits, max_distance,
                                (float)max_col_distance, (float)max_row_distance, plan.cur_per_block, plan.keys_clean, plan.matrix_cores,
                                plan.n_boxes > 0 ? reinterpret_cast<float4 *>(ctx->match_boxes) : nullptr};
    FTK_HIP(ctx, ftk::match_launch(plan, p, ctx->stream));
    return FTK_OK;
}

int ftk_hamming_match(ftk_context *ctx, const uint32_t *ref_words, int32_t n_ref, const uint32_t *cur_words, int32_t n_cur, int32_t n_words,
                      int32_t n_bits, float max_distance, const float *pred_uv, const float *cur_uv, int32_t max_col_distance,
                      int32_t max_row_distance, int32_t *index_pairs, int *matched_ok) {
    FTK_TRACE_SCOPE("ftk_hamming_match");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "hamming_match: null context");
    }
    FTK_LOCK(ctx);
    if (matched_ok) {
        *matched_ok = 0;
    }
    if (n_ref < 0 || n_cur < 0 || n_words < 1 || n_bits < 0 || n_bits > 32 * n_words) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "hamming_match: bad sizes (n_ref %d, n_cur %d, n_words %d, n_bits %d)", n_ref, n_cur, n_words, n_bits);
    }
    if (n_cur == 0) {
        return FTK_OK;  // descriptor_matcher.h:58 — `return false`
    }
    if (matched_ok) {
        *matched_ok = 1;
    }
    if (n_ref == 0) {
        return FTK_OK;
    }
    if (!ref_words || !cur_words || !index_pairs || (pred_uv && !cur_uv)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "hamming_match: null buffer");
    }
    const int32_t dev_words = ftk::hamming_device_words(n_words);  // padded on the host, during the gather
    return run_staged_match(ctx, ref_words, n_ref, cur_words, n_cur, sizeof(uint32_t) * n_words, sizeof(uint32_t) * dev_words, pred_uv, cur_uv, index_pairs,
                            [&](uint8_t *d_ref, uint8_t *d_cur, float *d_pred, float *d_cuv, int32_t *d_idx) {
                                return ftk_hamming_match_device(ctx, reinterpret_cast<uint32_t *>(d_ref), n_ref, reinterpret_cast<uint32_t *>(d_cur), n_cur,
                                                                dev_words, n_bits, max_distance, d_pred, d_cuv, max_col_distance, max_row_distance, d_idx, nullptr);
                            });
}

/* ---- diagnostics ---------------------------------------------------------------------------- */

int ftk_ldlt6_solve(ftk_context *ctx, const float *a, const float *b, float *x, int32_t n) {
    FTK_TRACE_SCOPE("ftk_ldlt6_solve");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "ldlt6_solve: null context");
    }
    FTK_LOCK(ctx);
    if (n < 0 || (n > 0 && (!a || !b || !x))) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "ldlt6_solve: bad arguments");
    }
    if (n == 0) {
        return FTK_OK;
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t a_bytes = align_up(sizeof(float) * 36 * (size_t)n, 256), b_bytes = align_up(sizeof(float) * 6 * (size_t)n, 256);
    const int rc = ftk_ensure_scratch(ctx, a_bytes + 2 * b_bytes);
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *base = static_cast<uint8_t *>(ctx->scratch);
    float *d_a = reinterpret_cast<float *>(base), *d_b = reinterpret_cast<float *>(base + a_bytes), *d_x = reinterpret_cast<float *>(base + a_bytes + b_bytes);
    FTK_HIP(ctx, hipMemcpyAsync(d_a, a, sizeof(float) * 36 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(d_b, b, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    FTK_HIP(ctx, ftk::ldlt6_launch(d_a, d_b, d_x, n, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(x, d_x, sizeof(float) * 6 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

/* ---- direct method ------------------------------------------------------------------------ */

void ftk_default_direct_options(ftk_direct_options *opt) {
    if (!opt) {
        return;
    }
    opt->max_track_points = 500;
    opt->max_iteration = 15;
    opt->half_rows = 6;
    opt->half_cols = 6;
    opt->max_converge_step = 1e-6f;
    opt->max_converge_residual = 2.0f;
    opt->method = FTK_METHOD_DIRECT;
}

namespace {

// The kernels' problem table from the caller's problems (checked here); *max_features: tracked features of the largest problem.
int direct_problem_table(ftk_context *ctx, const ftk_direct_options *opt, const ftk_direct_problem *problems, int32_t n_problems,
                         std::vector<ftk::DirectProblem> *table, uint32_t *max_features, int32_t *n_levels) {
    table->resize((size_t)n_problems);
    for (int32_t k = 0; k < n_problems; ++k) {
        const ftk_direct_problem &in = problems[k];
        if (!in.ref || !in.cur || in.n < 0 || (in.n > 0 && (!in.d_p_c_in_ref || !in.d_ref_uv || !in.d_cur_uv || !in.d_status)) || !in.d_pose) {
            return fail(ctx, FTK_E_INVALID_ARGUMENT, "direct_track: problem %d has a null buffer", k);
        }
        if (in.ref->n_levels != in.cur->n_levels || in.ref->n_levels < 1) {
            return fail(ctx, FTK_E_INVALID_ARGUMENT, "direct_track: problem %d pyramid level mismatch (%d vs %d)", k, in.ref->n_levels, in.cur->n_levels);
        }
        if (k == 0) {
            *n_levels = in.ref->n_levels;
        } else if (in.ref->n_levels != *n_levels) {
            return fail(ctx, FTK_E_UNSUPPORTED, "direct_track: all problems of a batch must share the pyramid depth");
        }
        if (in.ref->device != ctx->device || in.cur->device != ctx->device) {
            return fail(ctx, FTK_E_INVALID_ARGUMENT, "direct_track: pyramid lives on another device");
        }
        ftk::DirectProblem &out = (*table)[(size_t)k];
        memset(&out, 0, sizeof(out));
        memcpy(out.ref, in.ref->levels, sizeof(DevImage) * (size_t)*n_levels);
        memcpy(out.cur, in.cur->levels, sizeof(DevImage) * (size_t)*n_levels);
        memcpy(out.K, in.K, sizeof(out.K));
        out.p_ref = in.d_p_c_in_ref;
        out.ref_uv = in.d_ref_uv;
        out.cur_uv = in.d_cur_uv;
        out.pose = in.d_pose;
        out.status = in.d_status;
        out.iterations = in.d_iterations;
        out.n = in.n;
        out.status_valid = in.status_valid ? 1 : 0;
        const uint32_t tracked = ((uint32_t)in.n < opt->max_track_points) ? (uint32_t)in.n : opt->max_track_points;
        *max_features = std::max(*max_features, tracked);
    }
    return FTK_OK;
}

// The problem table travels through a context-owned device buffer (separate from the scratch the host-buffer wrapper uses); with the
// feature tables in device memory each problem gets its slice first.
int upload_direct_table(ftk_context *ctx, const ftk::DirectPlan &plan, std::vector<ftk::DirectProblem> &table) {
    const size_t n_problems = table.size();
    if (plan.feat_in_global) {
        const int rc = ensure_device_buffer(ctx, &ctx->direct_feat, &ctx->direct_feat_bytes, plan.feat_bytes * n_problems);
        if (rc != FTK_OK) {
            return rc;
        }
        for (size_t k = 0; k < n_problems; ++k) {
            table[k].feat = reinterpret_cast<float4 *>(static_cast<uint8_t *>(ctx->direct_feat) + plan.feat_bytes * k);
        }
    }
    const size_t table_bytes = sizeof(ftk::DirectProblem) * n_problems;
    if (table_bytes > ctx->direct_table_bytes) {
        if (ctx->direct_table) {
            FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            FTK_HIP(ctx, hipFree(ctx->direct_table));
            ctx->direct_table = nullptr;
            ctx->direct_table_bytes = 0;
        }
        FTK_HIP(ctx, hipMalloc(&ctx->direct_table, align_up(table_bytes, 4096)));
        ctx->direct_table_bytes = align_up(table_bytes, 4096);
    }
    // pageable host -> device copy: synchronous with respect to the host buffer, so `table` may go out of scope
    FTK_HIP(ctx, hipMemcpyAsync(ctx->direct_table, table.data(), table_bytes, hipMemcpyHostToDevice, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

// ftk_direct_track_batch_device; spread_allowed = false: the re-run of a poisoned spread launch on one workgroup per problem.
int direct_track_batch(ftk_context *ctx, const ftk_direct_options *opt, const ftk_direct_problem *problems, int32_t n_problems, bool spread_allowed) {
    if (!opt || n_problems < 0 || (n_problems > 0 && !problems)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "direct_track: null options / problems");
    }
    if (n_problems == 0) {
        return FTK_OK;
    }
    if (opt->half_rows < 0 || opt->half_cols < 0 || opt->half_rows > 63 || opt->half_cols > 63) {
        return fail(ctx, FTK_E_UNSUPPORTED, "direct_track: half patch size (%d, %d) outside [0, 63]", opt->half_rows, opt->half_cols);
    }
    std::vector<ftk::DirectProblem> table;
    uint32_t max_features = 0;
    int32_t n_levels = 0;
    int rc = direct_problem_table(ctx, opt, problems, n_problems, &table, &max_features, &n_levels);
    if (rc != FTK_OK) {
        return rc;
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const bool resident_known = ctx->direct_spread_resident >= 0 && ctx->direct_spread_resident_features == max_features;
    ftk::DirectPlanInput in = {n_problems, max_features, 2 * opt->half_rows + 1, 2 * opt->half_cols + 1, opt->method, ctx->reduction == FTK_REDUCTION_TREE,
                               spread_allowed, resident_known ? ctx->direct_spread_resident : ftk::kPlanNotSet, ftk::kPlanNotSet, ctx->direct_spread_bytes,
                               env_int(FTK_ENV(ctx, direct_spread)), env_int(FTK_ENV(ctx, direct_spread_resident)), env_int(FTK_ENV(ctx, direct_spread_poison)),
                               FTK_ENV(ctx, direct_spread_min_terms) ? atoll(FTK_ENV(ctx, direct_spread_min_terms)) : ftk::kPlanNotSet};
    ftk::DirectPlan plan = ftk::direct_plan(in);
    rc = upload_direct_table(ctx, plan, table);
    if (rc != FTK_OK) {
        return rc;
    }
    if (plan.ask_resident) {  // the occupancy query, cached per feature count
        ctx->direct_spread_resident = ftk::direct_spread_resident_groups(max_features, ctx->device);
        ctx->direct_spread_resident_features = max_features;
        in.resident = ctx->direct_spread_resident;
        plan = ftk::direct_plan(in);
    }
    if (plan.ask_capturing) {  // the spread workspace would grow: not inside a stream capture
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        in.capturing = hipStreamIsCapturing(ctx->stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
        plan = ftk::direct_plan(in);
    }
    ctx->direct_spread_launched = 0;
    if (plan.producers > 0) {
        rc = ensure_device_buffer(ctx, &ctx->direct_spread, &ctx->direct_spread_bytes, plan.ws_stride * (size_t)n_problems);
        if (rc != FTK_OK) {
            return rc;
        }
        for (int32_t k = 0; k < n_problems; ++k) {  // header + chunk flags of every problem: zero before the launch
            FTK_HIP(ctx, hipMemsetAsync(static_cast<uint8_t *>(ctx->direct_spread) + plan.ws_stride * (size_t)k, 0, plan.clear_bytes, ctx->stream));
        }
        ctx->direct_spread_launched = n_problems;
    }
    const ftk::DirectParams p = {static_cast<const ftk::DirectProblem *>(ctx->direct_table), in.tree, n_levels, opt->max_track_points, opt->max_iteration,
                                 opt->half_rows, opt->half_cols, in.patch_rows, in.patch_cols, opt->max_converge_step, opt->method, plan.producers,
                                 plan.producers > 0 ? static_cast<uint32_t *>(ctx->direct_spread) : nullptr, (uint32_t)(plan.ws_stride / sizeof(uint32_t)),
                                 plan.poison};
    FTK_HIP(ctx, ftk::direct_track_launch(plan, p, ctx->stream));
    return FTK_OK;
}

}  // namespace

int ftk_direct_track_batch_device(ftk_context *ctx, const ftk_direct_options *opt, const ftk_direct_problem *problems, int32_t n_problems) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "direct_track: null context");
    }
    FTK_LOCK(ctx);
    return direct_track_batch(ctx, opt, problems, n_problems, true);
}

int ftk_direct_track(ftk_context *ctx, const ftk_direct_options *opt, const ftk_pyramid *ref, const ftk_pyramid *cur, const float *K,
                     const float *p_c_in_ref, const float *ref_uv, float *cur_uv, int32_t n, float *q_rc_wxyz, float *p_rc, uint8_t *status,
                     int status_valid, uint32_t *iterations) {
    FTK_TRACE_SCOPE("ftk_direct_track");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "direct_track: null context");
    }
    FTK_LOCK(ctx);
    if (n < 0) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "direct_track: negative feature count");
    }
    if (n == 0) {
        return FTK_OK;  // the class returns false for an empty ref_pixel_uv (:38); nothing to compute here
    }
    if (!opt || !ref || !cur || !K || !p_c_in_ref || !ref_uv || !cur_uv || !q_rc_wxyz || !p_rc || !status) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "direct_track: null argument");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pts_bytes = align_up(sizeof(float) * 3 * (size_t)n, 256);
    const size_t uv_bytes = align_up(sizeof(float) * 2 * (size_t)n, 256);
    const size_t st_bytes = align_up((size_t)n, 256);
    const size_t total = pts_bytes + 2 * uv_bytes + st_bytes + 256 + 256;
    int rc = ftk_ensure_scratch(ctx, total);
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *base = static_cast<uint8_t *>(ctx->scratch);
    float *d_pts = reinterpret_cast<float *>(base);
    float *d_ref = reinterpret_cast<float *>(base + pts_bytes);
    float *d_cur = reinterpret_cast<float *>(base + pts_bytes + uv_bytes);
    uint8_t *d_st = base + pts_bytes + 2 * uv_bytes;
    float *d_pose = reinterpret_cast<float *>(base + pts_bytes + 2 * uv_bytes + st_bytes);
    uint32_t *d_it = reinterpret_cast<uint32_t *>(base + pts_bytes + 2 * uv_bytes + st_bytes + 256);
    float pose[7];
    auto upload_state = [&]() -> int {  // the in/out buffers: positions, statuses and the pose (`pose` is a stack buffer: synchronised)
        memcpy(pose, q_rc_wxyz, sizeof(float) * 4);
        memcpy(pose + 4, p_rc, sizeof(float) * 3);
        FTK_HIP(ctx, hipMemcpyAsync(d_cur, cur_uv, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        FTK_HIP(ctx, hipMemcpyAsync(d_st, status, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        FTK_HIP(ctx, hipMemcpyAsync(d_pose, pose, sizeof(pose), hipMemcpyHostToDevice, ctx->stream));
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FTK_OK;
    };
    FTK_HIP(ctx, hipMemcpyAsync(d_pts, p_c_in_ref, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(d_ref, ref_uv, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    rc = upload_state();
    if (rc != FTK_OK) {
        return rc;
    }
    const ftk_direct_problem prob = {ref, cur, {K[0], K[1], K[2], K[3]}, d_pts, d_ref, d_cur, n, d_pose, d_st, status_valid, d_it};
    rc = direct_track_batch(ctx, opt, &prob, 1, true);
    if (rc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    if (ctx->direct_spread_launched > 0) {
        // The spread kernel's bounded waits ran out (its 1 + NP workgroups were not co-resident: a CU mask, a partition smaller than the
        // runtime reported, long kernels of other streams): header word 1 is set and the pose is NaN.  A synchronous caller must never
        // get that with FTK_OK — run the problem again on the one-workgroup kernel (same sums, same result as a good spread launch).
        uint32_t poisoned = 0;
        FTK_HIP(ctx, hipMemcpyAsync(&poisoned, static_cast<uint32_t *>(ctx->direct_spread) + 1, sizeof(poisoned), hipMemcpyDeviceToHost, ctx->stream));
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (poisoned != 0) {
            rc = upload_state();
            rc = rc == FTK_OK ? direct_track_batch(ctx, opt, &prob, 1, false) : rc;
            if (rc != FTK_OK) {
                (void)hipStreamSynchronize(ctx->stream);
                return rc;
            }
            ++ctx->direct_spread_reruns;
            // not a failure — the result below is the one-workgroup kernel's — but worth telling: ftk_last_error() carries the note
            ctx->error = "note: ftk_direct_track: the spread launch was not co-resident (its bounded waits ran out); the problem was re-run on one workgroup";
        }
    }
    uint32_t it = 0;
    FTK_HIP(ctx, hipMemcpyAsync(cur_uv, d_cur, sizeof(float) * 2 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(status, d_st, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(pose, d_pose, sizeof(pose), hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(&it, d_it, sizeof(it), hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(q_rc_wxyz, pose, sizeof(float) * 4);
    memcpy(p_rc, pose + 4, sizeof(float) * 3);
    if (iterations) {
        *iterations = it;
    }
    return FTK_OK;
}

/* ---- float-descriptor matcher -------------------------------------------------------------- */

int ftk_cosine_match_device(ftk_context *ctx, const float *d_ref_desc, int32_t n_ref, const float *d_cur_desc, int32_t n_cur, int32_t dim,
                            float max_distance, const float *d_pred_uv, const float *d_cur_uv, int32_t max_col_distance,
                            int32_t max_row_distance, int32_t *d_index_pairs) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "cosine_match_device: null context");
    }
    FTK_LOCK(ctx);
    if (n_ref < 0 || n_cur < 0 || dim < 1) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "cosine_match_device: bad sizes (n_ref %d, n_cur %d, dim %d)", n_ref, n_cur, dim);
    }
    if (dim > 4096) {
        return fail(ctx, FTK_E_UNSUPPORTED, "cosine_match_device: dim %d > 4096", dim);
    }
    if (n_ref == 0 || n_cur == 0) {
        return FTK_OK;
    }
    if (!d_ref_desc || !d_cur_desc || !d_index_pairs || (d_pred_uv && !d_cur_uv)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "cosine_match_device: null buffer");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const ftk::CosinePlanInput in = {n_ref, n_cur, dim, d_pred_uv != nullptr, ((reinterpret_cast<uintptr_t>(d_ref_desc) | reinterpret_cast<uintptr_t>(d_cur_desc)) & 15u) == 0,
                                     env_int(FTK_ENV(ctx, cosine_small)), env_int(FTK_ENV(ctx, cosine_chunked)), env_int(FTK_ENV(ctx, cosine_splits))};
    const ftk::CosinePlan plan = ftk::cosine_plan(in);
    const int rc = ensure_device_buffer(ctx, &ctx->cosine_ws, &ctx->cosine_ws_bytes, plan.ws_bytes);
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *ws = static_cast<uint8_t *>(ctx->cosine_ws);
    auto at = [ws](size_t offset) { return reinterpret_cast<void *>(ws + offset); };
    const ftk::CosineParams p = {d_ref_desc, d_cur_desc, d_pred_uv, d_cur_uv, d_index_pairs, (_Float16 *)at(plan.ref_h), (_Float16 *)at(plan.cur_h),
                                 (float *)at(plan.ref_norm), (float *)at(plan.cur_norm), (float *)at(plan.cur_bias), (float4 *)at(plan.cur_info),
                                 plan.use_tile_box ? (float4 *)at(plan.tile_box) : nullptr, ws + plan.ref_irregular, (uint32_t *)at(plan.row_max),
                                 (uint32_t *)at(plan.cand_count), (int32_t *)at(plan.cand), plan.ref_stationary ? (float *)at(plan.cand_score) : nullptr,
                                 (uint32_t *)at(plan.irregular_count), (int32_t *)at(plan.irregular_list), at(plan.row_max), plan.clear_end - plan.row_max,
                                 n_ref, n_cur, dim, plan.n_ref_pad, plan.n_cur_pad, plan.dim_pad, plan.tiles_per_split, plan.ref_stationary, plan.splits,
                                 max_distance, (float)max_col_distance, (float)max_row_distance};
    FTK_HIP(ctx, ftk::cosine_match_launch(plan, p, ctx->stream));
    return FTK_OK;
}

int ftk_cosine_match(ftk_context *ctx, const float *ref_desc, int32_t n_ref, const float *cur_desc, int32_t n_cur, int32_t dim, float max_distance,
                     const float *pred_uv, const float *cur_uv, int32_t max_col_distance, int32_t max_row_distance, int32_t *index_pairs,
                     int *matched_ok) {
    FTK_TRACE_SCOPE("ftk_cosine_match");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "cosine_match: null context");
    }
    FTK_LOCK(ctx);
    if (matched_ok) {
        *matched_ok = 0;
    }
    if (n_ref < 0 || n_cur < 0 || dim < 1) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "cosine_match: bad sizes (n_ref %d, n_cur %d, dim %d)", n_ref, n_cur, dim);
    }
    if (n_cur == 0) {
        return FTK_OK;  // descriptor_matcher.h:58,94 — `return false`
    }
    if (matched_ok) {
        *matched_ok = 1;
    }
    if (n_ref == 0) {
        return FTK_OK;
    }
    if (!ref_desc || !cur_desc || !index_pairs || (pred_uv && !cur_uv)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "cosine_match: null buffer");
    }
    return run_staged_match(ctx, ref_desc, n_ref, cur_desc, n_cur, sizeof(float) * dim, sizeof(float) * dim, pred_uv, cur_uv, index_pairs,
                            [&](uint8_t *d_ref, uint8_t *d_cur, float *d_pred, float *d_cuv, int32_t *d_idx) {
                                return ftk_cosine_match_device(ctx, reinterpret_cast<float *>(d_ref), n_ref, reinterpret_cast<float *>(d_cur), n_cur, dim,
                                                               max_distance, d_pred, d_cuv, max_col_distance, max_row_distance, d_idx);
                            });
}

/* ---- dense optical flow (Farneback) ------------------------------------------------------------ */

void ftk_default_dense_flow_options(ftk_dense_flow_options *opt) {
    if (!opt) {
        return;
    }
    opt->max_iteration = 10;  // dense_optical_flow.h:15-20
    opt->half_patch = 2;
    opt->max_converge_step = 1e-6f;
    opt->max_delta_flow_step = 1.0f;
    opt->k_moments[0] = opt->k_moments[1] = opt->k_moments[2] = 0.0f;
}

int ftk_dense_flow_gaussian(int32_t half_patch, float *weights_out, float *k_out) {
    if (half_patch < 0 || half_patch > FTK_DENSE_MAX_HALF_PATCH) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "dense_flow_gaussian: half_patch %d outside [0, %d]", half_patch, FTK_DENSE_MAX_HALF_PATCH);
    }
    // InitializeGaussianKernel (dense_optical_flow.cpp:87-134)
    const int32_t center = half_patch, size = 2 * center + 1;
    std::vector<float> w((size_t)size * size, 0.0f);
    if (center == 0) {  // :95-98: [1], k2 / k4 / k22 not recomputed
        w[0] = 1.0f;
    } else {
        const float sigma = 1.0f, sigma2 = sigma * sigma;
        float sum = 0.0f;
        for (int32_t row = 0; row < size; ++row) {  // :106-113
            for (int32_t col = 0; col < size; ++col) {
                const int32_t dr = row - center, dc = col - center;
                w[(size_t)row * size + col] = expf(-0.5f * (float)(dr * dr + dc * dc) / sigma2);
                sum += w[(size_t)row * size + col];
            }
        }
        for (float &v : w) {  // :116
            v /= sum;
        }
        float k2 = 0.0f, k4 = 0.0f, k22 = 0.0f;  // :119-131, each product left to right
        for (int32_t row = 0; row < size; ++row) {
            for (int32_t col = 0; col < size; ++col) {
                const float fr = (float)(row - center), fc = (float)(col - center), wt = w[(size_t)row * size + col];
                k2 += wt * fr * fr;
                k4 += wt * fr * fr * fr * fr;
                k22 += wt * fr * fr * fc * fc;
            }
        }
        if (k_out) {
            k_out[0] = k2;
            k_out[1] = k4;
            k_out[2] = k22;
        }
    }
    if (weights_out) {
        memcpy(weights_out, w.data(), sizeof(float) * w.size());
    }
    return FTK_OK;
}

namespace {

bool stream_capturing(ftk_context *ctx) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cap) != hipSuccess) {
        return true;  // unknown: be safe
    }
    return cap != hipStreamCaptureStatusNone;
}

struct DenseLayout {
    float4 *mom_ref, *mom_cur;
    float *raw_r, *raw_c, *smooth_r, *smooth_c;
    float k[3];
};

// Checks the options and levels [lo, hi] of both pyramids, makes the Gaussian table resident and the workspace large enough
// (never inside a stream capture), and carves the workspace.
int dense_setup(ftk_context *ctx, const char *who, const ftk_dense_flow_options *opt, const ftk_pyramid *ref, const ftk_pyramid *cur, int32_t lo,
                int32_t hi, DenseLayout *L) {
    const int32_t half = opt->half_patch;
    size_t ref_px = 1, cur_px = 1;
    for (int32_t l = lo; l <= hi; ++l) {
        const DevImage a = ref->levels[l], b = cur->levels[l];
        if (a.rows <= 0 || a.cols <= 0 || b.rows <= 0 || b.cols <= 0 || !a.data || !b.data) {
            return fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: level %d is empty", who, l);
        }
        ref_px = std::max(ref_px, (size_t)a.rows * a.cols);
        cur_px = std::max(cur_px, (size_t)b.rows * b.cols);
    }
    const size_t mom_ref_bytes = align_up(2 * sizeof(float4) * ref_px, 256), mom_cur_bytes = align_up(2 * sizeof(float4) * cur_px, 256);
    const size_t plane_bytes = align_up(sizeof(float) * ref_px, 256);
    const size_t need = mom_ref_bytes + mom_cur_bytes + 4 * plane_bytes;
    const bool capturing = stream_capturing(ctx);
    if (need > ctx->dense_ws_bytes || ctx->dense_half != half) {
        if (capturing) {
            return fail(ctx, FTK_E_UNSUPPORTED, "%s: the workspace (%zu bytes) or the Gaussian table of half patch %d is not resident yet and "
                        "cannot be allocated while the stream is being captured: make one call of this shape and half patch before the capture", who,
                        need, half);
        }
    }
    std::vector<float> w((size_t)(2 * half + 1) * (2 * half + 1));
    L->k[0] = opt->k_moments[0];
    L->k[1] = opt->k_moments[1];
    L->k[2] = opt->k_moments[2];
    int rc = ftk_dense_flow_gaussian(half, w.data(), L->k);
    if (rc != FTK_OK) {
        return fail(ctx, rc, "%s: half_patch %d outside [0, %d]", who, half, FTK_DENSE_MAX_HALF_PATCH);
    }
    if (ctx->dense_half != half) {
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // earlier launches may still read the old table
        if (ctx->dense_weights) {
            FTK_HIP(ctx, hipFree(ctx->dense_weights));
            ctx->dense_weights = nullptr;
            ctx->dense_half = -1;
        }
        const size_t bytes = sizeof(float) * w.size();
        FTK_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->dense_weights), bytes));
        rc = ftk_ensure_pinned(ctx, bytes);
        if (rc != FTK_OK) {
            return rc;
        }
        memcpy(ctx->pinned, w.data(), bytes);
        FTK_HIP(ctx, hipMemcpyAsync(ctx->dense_weights, ctx->pinned, bytes, hipMemcpyHostToDevice, ctx->stream));
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the pinned block is reused by the caller right away
        ctx->dense_half = half;
    }
    if (need > ctx->dense_ws_bytes) {
        rc = ftk_ensure_device_buffer(ctx, &ctx->dense_ws, &ctx->dense_ws_bytes, need);
        if (rc != FTK_OK) {
            return rc;
        }
    }
    uint8_t *base = static_cast<uint8_t *>(ctx->dense_ws);
    L->mom_ref = reinterpret_cast<float4 *>(base);
    L->mom_cur = reinterpret_cast<float4 *>(base + mom_ref_bytes);
    float *planes = reinterpret_cast<float *>(base + mom_ref_bytes + mom_cur_bytes);
    const size_t pf = plane_bytes / sizeof(float);
    L->raw_r = planes;
    L->raw_c = planes + pf;
    L->smooth_r = planes + 2 * pf;
    L->smooth_c = planes + 3 * pf;
    return FTK_OK;
}

// One level: moments of ref and cur, the per-pixel refinement (initial flow per `init`), the median into out_r / out_c.
int dense_level(ftk_context *ctx, const ftk_dense_flow_options *opt, const DenseLayout &L, DevImage ref, DevImage cur, int32_t init, int32_t flow_valid,
                const float *init_r, const float *init_c, int32_t init_rows, int32_t init_cols, float *out_r, float *out_c) {
    ftk::DenseMomentsParams mp;
    mp.img[0] = ref;
    mp.img[1] = cur;
    mp.mom[0] = L.mom_ref;
    mp.mom[1] = L.mom_cur;
    mp.weights = ctx->dense_weights;
    mp.half = opt->half_patch;
    FTK_HIP(ctx, ftk::dense_moments_launch(mp, ctx->stream));
    ftk::DenseFlowParams fp;
    fp.mom_ref = L.mom_ref;
    fp.mom_cur = L.mom_cur;
    fp.ref_rows = ref.rows;
    fp.ref_cols = ref.cols;
    fp.cur_rows = cur.rows;
    fp.cur_cols = cur.cols;
    fp.k2 = L.k[0];
    fp.k4 = L.k[1];
    fp.k22 = L.k[2];
    fp.max_iteration = opt->max_iteration;
    fp.converge = opt->max_converge_step;
    fp.max_step = opt->max_delta_flow_step;
    fp.init = init;
    fp.flow_valid = flow_valid;
    fp.init_r = init_r;
    fp.init_c = init_c;
    fp.init_rows = init_rows;
    fp.init_cols = init_cols;
    fp.out_r = L.raw_r;
    fp.out_c = L.raw_c;
    FTK_HIP(ctx, ftk::dense_flow_launch(fp, ctx->stream));
    ftk::DenseMedianParams md;
    md.in_r = L.raw_r;
    md.in_c = L.raw_c;
    md.out_r = out_r;
    md.out_c = out_c;
    md.rows = ref.rows;
    md.cols = ref.cols;
    FTK_HIP(ctx, ftk::dense_median_launch(md, ctx->stream));
    return FTK_OK;
}

}  // namespace

int ftk_dense_flow_device(ftk_context *ctx, const ftk_dense_flow_options *opt, const ftk_pyramid *ref_pyr, const ftk_pyramid *cur_pyr, float *d_flow_r,
                          float *d_flow_c) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "dense_flow_device: null context");
    }
    FTK_LOCK(ctx);
    if (!opt || !ref_pyr || !cur_pyr || !d_flow_r || !d_flow_c) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "dense_flow_device: null argument");
    }
    if (ref_pyr->n_levels != cur_pyr->n_levels || ref_pyr->n_levels < 1) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "dense_flow_device: level counts %d and %d (the reference returns false unless they are equal)",
                    ref_pyr->n_levels, cur_pyr->n_levels);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const DevImage ref0 = ref_pyr->levels[0];
    if (opt->half_patch < 0) {
        // every per-level Track returns false before it touches the flow (:12) and the pyramid overload ignores it (:53): the
        // zero flow of the coarsest level, upsampled to level 0, is zero
        const size_t bytes = sizeof(float) * (size_t)ref0.rows * ref0.cols;
        FTK_HIP(ctx, hipMemsetAsync(d_flow_r, 0, bytes, ctx->stream));
        FTK_HIP(ctx, hipMemsetAsync(d_flow_c, 0, bytes, ctx->stream));
        return FTK_OK;
    }
    DenseLayout L;
    const int32_t top = ref_pyr->n_levels - 1;
    int rc = dense_setup(ctx, "dense_flow_device", opt, ref_pyr, cur_pyr, 0, top, &L);
    if (rc != FTK_OK) {
        return rc;
    }
    for (int32_t level = top; level >= 0; --level) {
        const DevImage coarse = ref_pyr->levels[level < top ? level + 1 : top];
        rc = dense_level(ctx, opt, L, ref_pyr->levels[level], cur_pyr->levels[level], level == top ? 0 : 2, 0, L.smooth_r, L.smooth_c, coarse.rows,
                         coarse.cols, level == 0 ? d_flow_r : L.smooth_r, level == 0 ? d_flow_c : L.smooth_c);
        if (rc != FTK_OK) {
            return rc;
        }
    }
    return FTK_OK;
}

int ftk_dense_flow(ftk_context *ctx, const ftk_dense_flow_options *opt, const ftk_pyramid *ref_pyr, const ftk_pyramid *cur_pyr, float *flow_r,
                   float *flow_c) {
    FTK_TRACE_SCOPE("ftk_dense_flow");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "dense_flow: null context");
    }
    FTK_LOCK(ctx);
    if (!ref_pyr || !flow_r || !flow_c || ref_pyr->n_levels < 1) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "dense_flow: null argument");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)ref_pyr->levels[0].rows * ref_pyr->levels[0].cols;
    const size_t plane = align_up(sizeof(float) * px, 256);
    int rc = ftk_ensure_scratch(ctx, 2 * plane);
    if (rc != FTK_OK) {
        return rc;
    }
    float *d_r = static_cast<float *>(ctx->scratch);
    float *d_c = reinterpret_cast<float *>(static_cast<uint8_t *>(ctx->scratch) + plane);
    rc = ftk_dense_flow_device(ctx, opt, ref_pyr, cur_pyr, d_r, d_c);
    if (rc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    rc = ftk_ensure_pinned(ctx, 2 * plane);
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *h = static_cast<uint8_t *>(ctx->pinned);
    FTK_HIP(ctx, hipMemcpyAsync(h, d_r, sizeof(float) * px, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(h + plane, d_c, sizeof(float) * px, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(flow_r, h, sizeof(float) * px);
    memcpy(flow_c, h + plane, sizeof(float) * px);
    return FTK_OK;
}

int ftk_dense_flow_level(ftk_context *ctx, const ftk_dense_flow_options *opt, const ftk_pyramid *ref_pyr, const ftk_pyramid *cur_pyr, int32_t level,
                         float *flow_r, float *flow_c, int32_t flow_valid) {
    FTK_TRACE_SCOPE("ftk_dense_flow_level");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "dense_flow_level: null context");
    }
    FTK_LOCK(ctx);
    if (!opt || !ref_pyr || !cur_pyr || !flow_r || !flow_c || level < 0 || level >= ref_pyr->n_levels || level >= cur_pyr->n_levels) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "dense_flow_level: bad arguments (level %d)", level);
    }
    if (opt->half_patch < 0) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "dense_flow_level: half_patch %d < 0 (the reference returns false, the flow untouched)", opt->half_patch);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    DenseLayout L;
    int rc = dense_setup(ctx, "dense_flow_level", opt, ref_pyr, cur_pyr, level, level, &L);
    if (rc != FTK_OK) {
        return rc;
    }
    const DevImage ref = ref_pyr->levels[level];
    const size_t px = (size_t)ref.rows * ref.cols, plane = align_up(sizeof(float) * px, 256);
    rc = ftk_ensure_pinned(ctx, 2 * plane);
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *h = static_cast<uint8_t *>(ctx->pinned);
    if (flow_valid & 1) {
        memcpy(h, flow_r, sizeof(float) * px);
        FTK_HIP(ctx, hipMemcpyAsync(L.raw_r, h, sizeof(float) * px, hipMemcpyHostToDevice, ctx->stream));
    }
    if (flow_valid & 2) {
        memcpy(h + plane, flow_c, sizeof(float) * px);
        FTK_HIP(ctx, hipMemcpyAsync(L.raw_c, h + plane, sizeof(float) * px, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = dense_level(ctx, opt, L, ref, cur_pyr->levels[level], 1, flow_valid & 3, L.raw_r, L.raw_c, ref.rows, ref.cols, L.smooth_r, L.smooth_c);
    if (rc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    FTK_HIP(ctx, hipMemcpyAsync(h, L.smooth_r, sizeof(float) * px, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(h + plane, L.smooth_c, sizeof(float) * px, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(flow_r, h, sizeof(float) * px);
    memcpy(flow_c, h + plane, sizeof(float) * px);
    return FTK_OK;
}

int ftk_fill_matched_pixels(const int32_t *index_pairs, int32_t n_ref, const float *cur_uv, int32_t n_cur, float *matched_uv, uint8_t *status) {
    if (n_ref < 0 || n_cur < 0 || (n_ref > 0 && (!index_pairs || !matched_uv || !status)) || (n_cur > 0 && !cur_uv)) {
        return FTK_E_INVALID_ARGUMENT;
    }
    for (int32_t i = 0; i < n_ref; ++i) {
        if (status[i] > FTK_TRACKED) {
            continue;
        }
        const int32_t j = index_pairs[i];
        if (j >= 0 && j < n_cur) {
            matched_uv[2 * i] = cur_uv[2 * j];
            matched_uv[2 * i + 1] = cur_uv[2 * j + 1];
            status[i] = FTK_TRACKED;
        } else {
            status[i] = FTK_LARGE_RESIDUAL;
        }
    }
    return FTK_OK;
}

// ---- RAFT correlation pyramid (correlation_volumes.py) ----

int ftk_corr_pyramid_layout(int32_t B, int32_t H, int32_t W, int32_t levels, int64_t *elements, int64_t *level_offsets, int32_t *level_h,
                            int32_t *level_w) {
    if (!elements) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_layout: null output");
    }
    if (B < 1 || H < 1 || W < 1) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_layout: sizes B %d, H %d, W %d must be positive", B, H, W);
    }
    if (levels < 1 || levels > FTK_CORR_MAX_LEVELS) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_layout: %d levels (1 .. %d)", levels, FTK_CORR_MAX_LEVELS);
    }
    const int64_t slabs = (int64_t)B * H * W;  // < 2^63: each factor < 2^31
    int64_t total = 0;
    int32_t h = H, w = W;
    for (int32_t l = 0; l < levels; ++l) {
        if (h == 0 || w == 0) {
            return fail(nullptr, FTK_E_INVALID_ARGUMENT,
                        "corr_pyramid_layout: level %d of a %d x %d volume would be %d x %d (the reference's avg_pool2d raises): use at most %d levels",
                        l, H, W, h, w, l);
        }
        const int64_t hw = (int64_t)h * w;
        if (slabs > (INT64_MAX - total) / hw) {
            return fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_layout: the volume of B %d, %d x %d, %d levels overflows int64", B, H, W, levels);
        }
        if (level_offsets) {
            level_offsets[l] = total;
        }
        if (level_h) {
            level_h[l] = h;
        }
        if (level_w) {
            level_w[l] = w;
        }
        total += slabs * hw;
        h /= 2;
        w /= 2;
    }
    if (total > INT64_MAX / 4) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_layout: %lld elements do not fit in a byte count", (long long)total);
    }
    *elements = total;
    return FTK_OK;
}

int ftk_corr_pyramid_build_device(ftk_context *ctx, void *stream, const float *d_fmap0, const float *d_fmap1, int32_t B, int32_t C, int32_t H,
                                  int32_t W, int32_t levels, float *d_volume) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_build_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_fmap0 || !d_fmap1 || !d_volume) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_build_device: null argument");
    }
    if (C < 1) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_build_device: %d channels", C);
    }
    int64_t elements = 0, off[FTK_CORR_MAX_LEVELS];
    int32_t lh[FTK_CORR_MAX_LEVELS], lw[FTK_CORR_MAX_LEVELS];
    if (ftk_corr_pyramid_layout(B, H, W, levels, &elements, off, lh, lw) != FTK_OK) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_build_device: %s", ftk_last_error(nullptr));
    }
    if ((int64_t)B * C * H * W > INT64_MAX / 4) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_build_device: feature maps too large");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    ftk::CorrBuildParams p{};
    p.f0 = d_fmap0;
    p.f1 = d_fmap1;
    p.volume = d_volume;
    p.B = B;
    p.C = C;
    p.H = H;
    p.W = W;
    p.divisor = (float)sqrt((double)C);  // correlation / (channels ** 0.5): a double scalar, cast to float by torch (:46)
    p.fused = std::min(levels - 1, ftk::corr_fused_levels());
    for (int l = 0; l < 4; ++l) {
        p.level_offset[l] = l < levels ? off[l] : 0;
        p.level_h[l] = l < levels ? lh[l] : 0;
        p.level_w[l] = l < levels ? lw[l] : 0;
    }
    FTK_HIP(ctx, ftk::corr_build_launch(p, s));
    // deeper levels (:31-34), each from the one before it
    const int64_t slabs = (int64_t)B * H * W;
    for (int32_t l = p.fused + 1; l < levels; ++l) {
        FTK_HIP(ctx, ftk::corr_pool_launch(d_volume + off[l - 1], d_volume + off[l], slabs, lh[l - 1], lw[l - 1], lh[l], lw[l], s));
    }
    return FTK_OK;
}

int ftk_corr_pyramid_lookup_device(ftk_context *ctx, void *stream, const float *d_volume, int32_t B, int32_t H, int32_t W, int32_t levels,
                                   int32_t radius, const float *d_coords, float *d_out, int32_t per_level) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_lookup_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_volume || !d_coords || !d_out) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_lookup_device: null argument");
    }
    if (radius < 0 || radius > FTK_CORR_MAX_RADIUS) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_lookup_device: radius %d (0 .. %d)", radius, FTK_CORR_MAX_RADIUS);
    }
    int64_t elements = 0;
    ftk::CorrLookupParams p{};
    if (ftk_corr_pyramid_layout(B, H, W, levels, &elements, p.level_offset, p.level_h, p.level_w) != FTK_OK) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_lookup_device: %s", ftk_last_error(nullptr));
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    p.volume = d_volume;
    p.coords = d_coords;
    p.out = d_out;
    p.B = B;
    p.H = H;
    p.W = W;
    p.levels = levels;
    p.radius = radius;
    p.per_level = per_level ? 1 : 0;
    FTK_HIP(ctx, ftk::corr_lookup_launch(p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

// ---- NNFeatureMatcher post-processing (nn_feature_matcher.cpp:155-216) ----

extern "C++" {
namespace {

// The key workspace of the nn_match entries, `count` 8-byte words, all 0.  It grows only outside a stream capture (an allocation is
// not a stream operation: a captured graph would keep launching on the freed block).
int ensure_nn_keys(ftk_context *ctx, const char *who, hipStream_t stream, size_t count) {
    if (count <= ctx->nn_keys_count) {
        return FTK_OK;
    }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return fail(ctx, FTK_E_UNSUPPORTED, "%s: the key workspace holds %zu words and this call needs %zu, and it cannot grow while the stream is being "
                    "captured: make one call of this size (or larger) on this context before the capture", who, ctx->nn_keys_count, count);
    }
    FTK_HIP(ctx, hipDeviceSynchronize());  // earlier calls, on whatever stream, may still use the old block
    if (ctx->nn_keys) {
        FTK_HIP(ctx, hipFree(ctx->nn_keys));
        ctx->nn_keys = nullptr;
        ctx->nn_keys_count = 0;
    }
    const size_t want = align_up(count + count / 4, 512);
    FTK_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->nn_keys), sizeof(unsigned long long) * want));
    FTK_HIP(ctx, hipMemset(ctx->nn_keys, 0, sizeof(unsigned long long) * want));  // 0 = empty; every call leaves it so
    FTK_HIP(ctx, hipDeviceSynchronize());
    ctx->nn_keys_count = want;
    return FTK_OK;
}

}  // namespace
}  // extern "C++"

int ftk_nn_match_scores_device(ftk_context *ctx, void *stream, const float *d_scores, int32_t batch, int32_t n_ref, int32_t n_cur, int64_t row_stride,
                               int64_t batch_stride, float min_score, int32_t *d_match_index, uint8_t *d_status) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: null context");
    }
    FTK_LOCK(ctx);
    if (batch < 0 || n_ref < 0 || n_cur < 0) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: negative size (batch %d, n_ref %d, n_cur %d)", batch, n_ref, n_cur);
    }
    if (batch == 0 || n_ref == 0) {
        return FTK_OK;  // nothing to write (nn_feature_matcher.cpp:92 returns false on an empty reference set: the callers' business)
    }
    if (n_cur == 0) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: n_cur 0 with n_ref %d: a row of no scores has no maximum (the reference would read "
                    "scores(0) of an empty row)", n_ref);
    }
    if (!d_scores || !d_match_index || !d_status) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: null buffer");
    }
    // rows may not overlap: row_stride >= n_cur, batch_stride >= the extent of one item; the whole extent must fit a byte count
    if (row_stride < n_cur || (n_ref > 1 && row_stride > INT64_MAX / 8 / n_ref)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: row stride %lld for %d x %d scores", (long long)row_stride, n_ref, n_cur);
    }
    const int64_t item = (int64_t)(n_ref - 1) * row_stride + n_cur;
    if (batch > 1 && (batch_stride < item || batch_stride > INT64_MAX / 8 / batch)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: batch stride %lld below the %lld elements of one item (or too large)",
                    (long long)batch_stride, (long long)item);
    }
    const ftk::NnMatchPlan plan = ftk::nn_match_plan({batch, n_ref, n_cur, row_stride, batch > 1 ? batch_stride : 0,
                                                      (reinterpret_cast<uintptr_t>(d_scores) & 15u) == 0});
    if (!plan.ok) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: batch %d x (%d + %d) does not fit one launch (batch <= %d, batch * (n_ref + n_cur) < 2^31)",
                    batch, n_ref, n_cur, ftk::kNnMaxBatch);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = ensure_nn_keys(ctx, "nn_match_scores_device", s, plan.key_count);
    if (rc != FTK_OK) {
        return rc;
    }
    ftk::NnMatchParams p{};
    p.scores = d_scores;
    p.row_stride = row_stride;
    p.batch_stride = batch > 1 ? batch_stride : 0;
    p.batch = batch;
    p.n_ref = n_ref;
    p.n_cur = n_cur;
    p.tile_rows = plan.tile_rows;
    p.col_tiles = plan.col_tiles;
    p.min_score = min_score;
    p.row_key = ctx->nn_keys;
    p.col_key = ctx->nn_keys + (size_t)batch * n_ref;
    p.done = reinterpret_cast<unsigned int *>(ctx->nn_keys + (size_t)batch * ((size_t)n_ref + n_cur));
    p.match_index = d_match_index;
    p.status = d_status;
    FTK_HIP(ctx, ftk::nn_match_scores_launch(plan, p, s));
    return FTK_OK;
}

int ftk_nn_match_list_device(ftk_context *ctx, void *stream, const int64_t *d_matches, int32_t n_matches, int32_t n_ref, int32_t n_cur,
                             int32_t *d_match_index, uint8_t *d_status) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "nn_match_list_device: null context");
    }
    FTK_LOCK(ctx);
    if (n_matches < 0 || n_ref < 0 || n_cur < 0 || n_matches == INT32_MAX) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_list_device: bad size (%d matches, n_ref %d, n_cur %d)", n_matches, n_ref, n_cur);
    }
    if (n_ref == 0) {
        return FTK_OK;
    }
    if (!d_match_index || !d_status || (n_matches > 0 && !d_matches)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_list_device: null buffer");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = ensure_nn_keys(ctx, "nn_match_list_device", s, (size_t)n_ref);
    if (rc != FTK_OK) {
        return rc;
    }
    FTK_HIP(ctx, ftk::nn_match_list_launch(reinterpret_cast<const long long *>(d_matches), n_matches, n_ref, n_cur, ctx->nn_keys, d_match_index, d_status, s));
    return FTK_OK;
}

int ftk_nn_fill_pixels_device(ftk_context *ctx, void *stream, const int32_t *d_match_index, int32_t n_ref, const float *d_cur_uv, int32_t n_cur,
                              float *d_matched_uv) {
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "nn_fill_pixels_device: null context");
    }
    FTK_LOCK(ctx);
    if (n_ref < 0 || n_cur < 0) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_fill_pixels_device: negative size (n_ref %d, n_cur %d)", n_ref, n_cur);
    }
    if (n_cur == 0) {
        return FTK_OK;  // matched_uv has n_cur entries
    }
    if (!d_cur_uv || !d_matched_uv || (n_ref > 0 && !d_match_index)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_fill_pixels_device: null buffer");
    }
    if (d_cur_uv == d_matched_uv) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_fill_pixels_device: matched_uv must not alias cur_uv (entries are gathered from cur_uv)");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::nn_fill_pixels_launch(d_match_index, n_ref, d_cur_uv, n_cur, d_matched_uv, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

extern "C++" {
namespace {

// The host-array forms: `in_bytes` of input go up, `launch(d_in, d_index, d_status)` runs on the context's stream, n_ref indices and
// statuses come back.  Synchronous.
template <class Launch>
int run_nn_host(ftk_context *ctx, const void *in, size_t in_bytes, int64_t n_out, int32_t *match_index, uint8_t *status, Launch launch) {
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t in_pad = align_up(in_bytes, 256), idx_pad = align_up(sizeof(int32_t) * (size_t)n_out, 256);
    const int rc = ftk_ensure_scratch(ctx, in_pad + idx_pad + (size_t)n_out);
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *base = static_cast<uint8_t *>(ctx->scratch);
    if (in_bytes > 0) {
        FTK_HIP(ctx, hipMemcpyAsync(base, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    int32_t *d_idx = reinterpret_cast<int32_t *>(base + in_pad);
    uint8_t *d_st = base + in_pad + idx_pad;
    const int lrc = launch(base, d_idx, d_st);
    if (lrc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return lrc;
    }
    FTK_HIP(ctx, hipMemcpyAsync(match_index, d_idx, sizeof(int32_t) * (size_t)n_out, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(status, d_st, (size_t)n_out, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

}  // namespace
}  // extern "C++"

int ftk_nn_match_scores(ftk_context *ctx, const float *scores, int32_t batch, int32_t n_ref, int32_t n_cur, int64_t row_stride, int64_t batch_stride,
                        float min_score, int32_t *match_index, uint8_t *status, int *matched_ok) {
    FTK_TRACE_SCOPE("ftk_nn_match_scores");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "nn_match_scores: null context");
    }
    FTK_LOCK(ctx);
    if (matched_ok) {
        *matched_ok = 0;
    }
    if (batch < 0 || n_ref < 0 || n_cur < 0) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores: negative size (batch %d, n_ref %d, n_cur %d)", batch, n_ref, n_cur);
    }
    if (n_ref == 0 || batch == 0) {
        return FTK_OK;  // nn_feature_matcher.cpp:92 — `return false`
    }
    if (n_cur == 0) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores: n_cur 0 with n_ref %d: a row of no scores has no maximum (the reference would read "
                    "scores(0) of an empty row)", n_ref);
    }
    if (!scores || !match_index || !status) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores: null buffer");
    }
    if (row_stride < n_cur || (n_ref > 1 && row_stride > INT64_MAX / 8 / n_ref)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores: row stride %lld for %d x %d scores", (long long)row_stride, n_ref, n_cur);
    }
    const int64_t item = (int64_t)(n_ref - 1) * row_stride + n_cur;
    if (batch > 1 && (batch_stride < item || batch_stride > INT64_MAX / 8 / batch)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores: batch stride %lld below the %lld elements of one item (or too large)",
                    (long long)batch_stride, (long long)item);
    }
    if ((int64_t)batch * n_ref >= (1ll << 31)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores: batch %d x n_ref %d does not fit one launch", batch, n_ref);
    }
    const int64_t extent = (batch > 1 ? (int64_t)(batch - 1) * batch_stride : 0) + item;  // elements from the first score to the last
    const int rc = run_nn_host(ctx, scores, sizeof(float) * (size_t)extent, (int64_t)batch * n_ref, match_index, status,
                               [&](uint8_t *d_in, int32_t *d_idx, uint8_t *d_st) {
                                   return ftk_nn_match_scores_device(ctx, ctx->stream, reinterpret_cast<float *>(d_in), batch, n_ref, n_cur, row_stride,
                                                                     batch_stride, min_score, d_idx, d_st);
                               });
    if (rc == FTK_OK && matched_ok) {
        *matched_ok = 1;
    }
    return rc;
}

int ftk_nn_match_list(ftk_context *ctx, const int64_t *matches, int32_t n_matches, int32_t n_ref, int32_t n_cur, int32_t *match_index, uint8_t *status,
                      int *matched_ok) {
    FTK_TRACE_SCOPE("ftk_nn_match_list");
    if (!ctx) {
        return fail(nullptr, FTK_E_INVALID_ARGUMENT, "nn_match_list: null context");
    }
    FTK_LOCK(ctx);
    if (matched_ok) {
        *matched_ok = 0;
    }
    if (n_matches < 0 || n_ref < 0 || n_cur < 0 || n_matches == INT32_MAX) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_list: bad size (%d matches, n_ref %d, n_cur %d)", n_matches, n_ref, n_cur);
    }
    if (n_ref == 0) {
        return FTK_OK;  // nn_feature_matcher.cpp:92 — `return false`
    }
    if (!match_index || !status || (n_matches > 0 && !matches)) {
        return fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_list: null buffer");
    }
    const int rc = run_nn_host(ctx, matches, sizeof(int64_t) * 2 * (size_t)n_matches, n_ref, match_index, status,
                               [&](uint8_t *d_in, int32_t *d_idx, uint8_t *d_st) {
                                   return ftk_nn_match_list_device(ctx, ctx->stream, reinterpret_cast<int64_t *>(d_in), n_matches, n_ref, n_cur, d_idx, d_st);
                               });
    if (rc == FTK_OK && matched_ok) {
        *matched_ok = 1;
    }
    return rc;
}

}  // extern "C"
