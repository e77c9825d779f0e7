// ftk_context.cpp — the context behind the C ABI (include/ftk.h): errors, create / destroy, synchronise, the FTK_* switches, warm-up.
//
// Host-side plumbing only: argument validation, device buffers, stream ordering, launches.
// All numerics live in the kernels.  There is deliberately no CPU fallback: if HIP is not
// usable every compute entry point fails with FTK_E_NO_DEVICE / FTK_E_HIP.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <string>

#include "ftk_internal.h"

namespace {
thread_local std::string g_create_error;  // ftk_last_error(NULL)
}  // namespace

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
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "context: null output pointer");
    }
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        return ftk_fail(nullptr, FTK_E_NO_DEVICE, "context: no HIP device available (%s); this library has no CPU fallback",
                        e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    }
    if (device < 0) {
        FTK_HIP(nullptr, hipGetDevice(&device));
    }
    if (device >= count) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "context: device %d out of range (have %d)", device, count);
    }
    FTK_HIP(nullptr, hipSetDevice(device));
    ftk_context *ctx = new (std::nothrow) ftk_context();
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_OUT_OF_MEMORY, "context: host allocation failed");
    }
    ctx->device = device;
    if (stream) {
        ctx->stream = reinterpret_cast<hipStream_t>(stream);
        ctx->owns_stream = false;
    } else {
        hipError_t se = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (se != hipSuccess) {
            delete ctx;
            return ftk_fail(nullptr, FTK_E_HIP, "context: hipStreamCreate failed: %s", hipGetErrorString(se));
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
    const hipStream_t owned_stream = ctx->owns_stream ? ctx->stream : nullptr;
    delete ctx;  // every block goes with its ftk_buffer member: after the synchronisation, before the stream
    if (owned_stream) {
        (void)hipStreamDestroy(owned_stream);
    }
}

const char *ftk_last_error(const ftk_context *ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int ftk_synchronize(ftk_context *ctx) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "synchronize: null context");
    }
    FTK_LOCK(ctx);
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

int ftk_context_refresh_env(ftk_context *ctx) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "context_refresh_env: null context");
    }
    FTK_LOCK(ctx);
    ctx->env.read();
    return FTK_OK;
}

int ftk_set_reduction_mode(ftk_context *ctx, int mode) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "set_reduction_mode: null context");
    }
    FTK_LOCK(ctx);
    if (mode != FTK_REDUCTION_EXACT && mode != FTK_REDUCTION_TREE) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "set_reduction_mode: unknown mode %d", mode);
    }
    ctx->reduction = mode;
    return FTK_OK;
}

int ftk_warmup(ftk_context *ctx, unsigned what) {
    FTK_TRACE_SCOPE("ftk_warmup");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "warmup: null context");
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
            rc = ftk_acquire_image_stage(ctx, 1u << 20, &stage);
        }
        if (rc != FTK_OK) {
            return rc;
        }
    }
    if (what & FTK_WARM_HAMMING) {
        FTK_HIP(ctx, ftk::matcher_warm(ctx->stream));
        FTK_HIP(ctx, ftk::feature_warm(ctx->stream));  // BRIEF descriptors sit in front of the matcher
        int rc = ftk_ensure_match_keys(ctx, 4096);
        if (rc == FTK_OK) {
            rc = ftk_ensure_scratch(ctx, 4u << 20);
        }
        if (rc == FTK_OK) {
            rc = ftk_ensure_pinned(ctx, 4u << 20);
        }
        if (rc == FTK_OK) {
            rc = ftk_ensure_brief_pattern(ctx, 256, 8);  // kLength / kHalfPatchSize of the reference's caller (test_descriptor_matcher_brief.cpp:71-72)
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
        const size_t probe = ctx->pinned.bytes() < ctx->scratch.bytes() ? ctx->pinned.bytes() : ctx->scratch.bytes();
        FTK_HIP(ctx, hipMemcpyAsync(ctx->scratch.get(), ctx->pinned.get(), probe, hipMemcpyHostToDevice, ctx->stream));
        FTK_HIP(ctx, hipMemcpyAsync(ctx->pinned.get(), ctx->scratch.get(), probe, hipMemcpyDeviceToHost, ctx->stream));
        void *tmp = nullptr;  // and one image-sized allocation: what every ftk_pyramid_upload / ftk_pyramid_build makes
        if (hipMalloc(&tmp, 4u << 20) == hipSuccess) {
            (void)hipFree(tmp);
        }
    }
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

}  // extern "C"
