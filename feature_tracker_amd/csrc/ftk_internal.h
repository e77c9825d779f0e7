// ftk_internal.h — definitions shared by the translation units behind the C ABI (ftk_context.cpp and one ftk_*.cpp per family of entry points).
// Not installed, not part of the boundary: include/ftk.h is.
#pragma once

#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <mutex>
#include <string>

#include "ftk_buffer.h"
#include "ftk_device.h"
#include "ftk_layout.h"
#include "klt_sched.h"

using ftk::DevImage;

// The FTK_* experiment switches of the library, read ONCE per context (ftk_context_create; ftk_context_refresh_env re-reads them for
// a test or a sweep that flips one): no getenv on any call path.  Most pick launch shapes and kernels and leave every result as it is.
// Two do not: FTK_REDUCTION=tree starts the context in the throughput mode (not the reference's summation order), and
// FTK_DIRECT_SPREAD_POISON=1 makes the spread direct-method kernel act as if its waits had run out (tests only).
#define FTK_ENV_SWITCHES(X)                                                                                                        \
    X(klt_waves, "FTK_KLT_WAVES") X(klt_group, "FTK_KLT_GROUP") X(lssd_chunked, "FTK_LSSD_CHUNKED") X(klt_spill, "FTK_KLT_SPILL")              \
    X(klt_spill_budget_mb, "FTK_KLT_SPILL_BUDGET_MB") X(klt_sched, "FTK_KLT_SCHED") X(klt_sched_min, "FTK_KLT_SCHED_MIN")                     \
    X(klt_sched_dump, "FTK_KLT_SCHED_DUMP") X(klt_swap_dump, "FTK_KLT_SWAP_DUMP") X(klt_tail_class, "FTK_KLT_TAIL_CLASS")                     \
    X(match_small, "FTK_MATCH_SMALL") X(match_kernel, "FTK_MATCH_KERNEL")                                                                  \
    X(direct_spread, "FTK_DIRECT_SPREAD") X(direct_spread_min_terms, "FTK_DIRECT_SPREAD_MIN_TERMS")                                        \
    X(direct_spread_resident, "FTK_DIRECT_SPREAD_RESIDENT") X(direct_spread_poison, "FTK_DIRECT_SPREAD_POISON")                            \
    X(cosine_small, "FTK_COSINE_SMALL") X(cosine_chunked, "FTK_COSINE_CHUNKED") X(cosine_splits, "FTK_COSINE_SPLITS")                      \
    X(reduction, "FTK_REDUCTION")

struct ftk_env {
#define X(field, name) const char *field = nullptr;
    FTK_ENV_SWITCHES(X)
#undef X
    enum { kCount = 0
#define X(field, name) +1
    FTK_ENV_SWITCHES(X)
#undef X
    };
    std::string keep[kCount];  // the values' storage: the environment may change under a pointer getenv returned
    void read() {
        int k = 0;
#define X(field, name)                     \
    if (const char *v = getenv(name)) {    \
        keep[k] = v;                       \
        field = keep[k].c_str();           \
    } else {                               \
        field = nullptr;                   \
    }                                      \
    ++k;
        FTK_ENV_SWITCHES(X)
#undef X
    }
    static bool off(const char *v) { return v && atoi(v) == 0; }  // "FTK_X=0" switches a default-on feature off
    static bool on(const char *v) { return v && atoi(v) != 0; }
};

#define FTK_ENV(ctx, field) ((ctx) ? (ctx)->env.field : nullptr)

struct ftk_context {
    // Every entry point that takes a context holds this lock for its whole duration: the scratch / pinned / workspace
    // buffers below are reused (and regrown) by every call, so calls on ONE context from several threads — e.g. the
    // left and right tracker objects of a stereo front end, which share the process-wide context of the C++ classes —
    // are serialised here instead of racing on them.  Recursive: the host-buffer wrappers call the *_device entries.
    std::recursive_mutex lock;
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    std::string error;
    ftk_env env;  // the experiment switches as they were when the context was made (or last refreshed)
    // Every block below is an ftk_buffer: it grows where it is used and goes with the context (ftk_context_destroy frees none by name).
    ftk_buffer scratch;      // cached device scratch for the host-buffer entry points
    ftk_buffer match_keys;   // 8-byte keys of the Hamming matcher: all ones = "no match yet" between calls
    ftk_buffer nn_keys;      // 8-byte keys of NNFeatureMatcher's post-processing (ftk_nn_match_*_device): all 0 = empty between calls; grown only outside a stream capture
    ftk_buffer match_boxes;  // NearbyMatch bounding boxes (4 floats each)
    ftk_buffer cosine_ws;    // workspace of the float-descriptor matcher (fp16 copies, norms, candidate lists)
    ftk_buffer direct_table; // problem table of the direct-method launches
    ftk_buffer direct_feat;  // per-feature projection tables of direct-method problems too large for LDS (16 B per tracked feature)
    // launch order of the trackers (ftk_klt_track_device): iteration counts of the last two calls and the permutations the
    // sort block of the tracker launches makes from them, double-buffered
    ftk_buffer sched_iters[2];  // uint32_t
    ftk_buffer sched_order[2];  // int32_t
    // position-keyed slot swaps (klt_order.h sched_resolve_slot): iteration counts by position (two hash tables), one claim word per launch slot
    ftk_buffer sched_grid, sched_claim;  // uint32_t
    ftk_buffer sched_pred;            // uint8_t: predicted iteration count of every feature of the call in hand (position-keyed launch order)
    ftk::KltSchedState sched;         // which order the next call gets (klt_sched.h klt_sched_step)
    // Tail-aware wave policy (round 5): the trackers' kernels report the iteration count of a call's LONGEST feature (features below
    // kTailReportFrom stay silent) into a device word per variant (atomicMax) whose raisers forward it to `tail_host`, device-visible host words
    // a later call's policy reads without any synchronisation: {call number << 8 | iterations}; feature 0 always reports, so every launch refreshes its word.  A heuristic input, never a result.
    ftk_buffer tail_host{ftk_buffer::kPinned}, tail_dev;  // 16 uint32_t each; allocated by a context's first tracker call outside a stream capture
    ftk::KltTailState tail;                 // launch numbers and the variants' tail classes (klt_sched.h klt_tail_class_step)
    ftk_buffer match_pad;      // zero-padded copies of descriptors whose width is not a power of two (device-resident matcher entry)
    ftk_buffer klt_spill;      // per-workgroup slices of the trackers' large-patch form (ftk_device.h KltParams::spill)
    ftk_buffer direct_spread;  // hand-off workspace of the spread direct-method kernel (header, chunk flags, products)
    int direct_spread_resident = -1;            // workgroups of the spread kernel this device holds at once (-1: not asked yet)
    uint32_t direct_spread_resident_features = 0;
    int direct_spread_launched = 0;             // problems the LAST ftk_direct_track_batch_device call spread over the chip (0: one workgroup each; header word 1 != 0: its waits ran out)
    uint32_t direct_spread_reruns = 0;          // such re-runs so far (tests)
    // pinned host staging for the host-buffer entry points (one H2D + one D2H per call)
    ftk_buffer pinned{ftk_buffer::kPinnedNonCoherent};
    // dense optical flow: moment images + flow planes (grown only outside a stream capture) and the Gaussian table (floats) of dense_half
    ftk_buffer dense_ws, dense_weights;
    int32_t dense_half = -1;
    // BRIEF sampling pattern (int8_t) resident on the device, cached per (n_bits, half)
    ftk_buffer brief_pattern;
    int32_t brief_bits = 0, brief_half = 0;
    // FTK_REDUCTION_EXACT (default) or FTK_REDUCTION_TREE: how the trackers' normal-equation sums are formed (ftk_set_reduction_mode)
    int32_t reduction = 0;
    // Two pinned, device-visible slots through which host images reach the pyramid launches (ftk_pyramid_build / _update of a
    // pageable image: a CPU copy into the slot, then the launch reads the slot over PCIe — no staged hipMemcpy, no stream
    // synchronisation; a slot is reused only after the event recorded behind its last reader has passed)
    struct ImageStage {
        ftk_buffer host{ftk_buffer::kPinned};
        const uint8_t *device_view = nullptr;
        hipEvent_t done = nullptr;
        bool busy = false;
        ~ImageStage() {
            if (done) {
                (void)hipEventDestroy(done);
            }
        }
    } image_stage[2];
    int image_stage_next = 0;
};

struct ftk_pyramid {
    int device = 0;
    int32_t n_levels = 0;
    DevImage levels[FTK_MAX_LEVELS];
    ftk_buffer owned;  // single allocation holding every owned level
};


// Records the message on the context (or, with ctx == nullptr, for ftk_last_error(NULL)) and returns `code`.
int ftk_fail(ftk_context *ctx, int code, const char *fmt, ...);

// The argument checks the entries share.  A null pointer is aligned: "may be null" and "must be aligned" are separate questions.
inline bool ftk_aligned(const void *p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }
inline bool ftk_finite(float v) { return v - v == 0.0f; }  // false for NaN and the infinities alone
inline bool ftk_positive(float v) { return v > 0.0f && ftk_finite(v); }

// The body of every ftk_*_workspace_bytes entry: `plan_call(&plan)` plans the call and answers FTK_OK or the refusal it has recorded.
template <class Plan, class PlanCall>
int ftk_workspace_bytes(const char *who, int64_t *bytes, PlanCall plan_call) {
    if (!bytes) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "%s: null argument", who);
    }
    Plan plan;
    const int rc = plan_call(&plan);
    if (rc == FTK_OK) {
        *bytes = (int64_t)plan.bytes;
    }
    return rc;
}

#define FTK_HIP(ctx, expr)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) {                                                                              \
            return ftk_fail(ctx, e_ == hipErrorOutOfMemory ? FTK_E_OUT_OF_MEMORY : FTK_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
        }                                                                                                    \
    } while (0)

#define FTK_LOCK(ctx) std::lock_guard<std::recursive_mutex> ftk_lock_guard_((ctx)->lock)

// FTK_TRACE=1 in the environment: every host-buffer entry point of the C ABI prints its wall time to stderr when it returns
// ("[ftk trace] ftk_klt_track 83.1 us") — for finding out where a caller's timed region goes; costs one getenv per process.
struct ftk_trace_scope {
    const char *name;
    std::chrono::steady_clock::time_point t0;
    bool on;
    explicit ftk_trace_scope(const char *n) : name(n), on(enabled()) {
        if (on) {
            t0 = std::chrono::steady_clock::now();
        }
    }
    ~ftk_trace_scope() {
        if (on) {
            fprintf(stderr, "[ftk trace] %s %.1f us\n", name, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        }
    }
    static bool enabled() {
        static const bool e = getenv("FTK_TRACE") != nullptr && atoi(getenv("FTK_TRACE")) != 0;
        return e;
    }
};
#define FTK_TRACE_SCOPE(name) ftk_trace_scope ftk_trace_scope_(name)

// Is `stream` being captured into a graph?  The one place that asks; a query that fails counts as capturing (allocating,
// synchronising or numbering a launch inside a capture is the mistake to avoid, refusing outside one merely costs a retry).
inline bool ftk_stream_capturing(hipStream_t stream) {
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &status) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    return status != hipStreamCaptureStatusNone;
}

// Growth policies of the context's blocks (they decide when a call reallocates, and so first-call times).  The device scratch /
// pinned host staging block of the host-buffer entry points: + 50 %, whole pages.
inline int ftk_ensure_scratch(ftk_context *ctx, size_t bytes) {
    FTK_HIP(ctx, ctx->scratch.reserve(ctx->stream, bytes, bytes / 2, 4096));
    return FTK_OK;
}
// (Coarse-grained, non-coherent host memory: cacheable in the device's L2, coherent at kernel boundaries — which is all the
// host-buffer entry points need: the host writes the block before the launch and reads it after the synchronisation.  The 2 000
// workgroups of a zero-copy tracker call then share 64-byte lines instead of each crossing PCIe for its own 17 bytes, and their
// results leave the chip as whole lines when the kernel ends: 2 000-feature call 68.1 / 71.2 -> 66.2 / 65.6 us, small calls unchanged.)
inline int ftk_ensure_pinned(ftk_context *ctx, size_t bytes) {
    FTK_HIP(ctx, ctx->pinned.reserve(ctx->stream, bytes, bytes / 2, 4096));
    return FTK_OK;
}
// Every other workspace that grows with the call: + 25 %, whole pages.
inline int ftk_ensure_device_buffer(ftk_context *ctx, ftk_buffer &buf, size_t bytes) {
    FTK_HIP(ctx, buf.reserve(ctx->stream, bytes, bytes / 4, 4096));
    return FTK_OK;
}

// The same three for a block carved by a staging layout (ftk_layout.h).  A layout whose sizes wrapped is refused here, before anything is sized by it.
inline int ftk_layout_refused(ftk_context *ctx) { return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "the array sizes of this call overflow its staging block"); }
inline int ftk_ensure_scratch(ftk_context *ctx, const ftk_layout &L) { return L.ok() ? ftk_ensure_scratch(ctx, L.bytes()) : ftk_layout_refused(ctx); }
inline int ftk_ensure_pinned(ftk_context *ctx, const ftk_layout &L) { return L.ok() ? ftk_ensure_pinned(ctx, L.bytes()) : ftk_layout_refused(ctx); }
inline int ftk_ensure_device_buffer(ftk_context *ctx, ftk_buffer &buf, const ftk_layout &L) {
    return L.ok() ? ftk_ensure_device_buffer(ctx, buf, L.bytes()) : ftk_layout_refused(ctx);
}
// The device scratch block and its pinned mirror, both laid out by `L` (the tracker, the matchers, BRIEF, dense flow).
inline int ftk_ensure_mirror(ftk_context *ctx, const ftk_layout &L, uint8_t **dbase, uint8_t **hbase) {
    int rc = ftk_ensure_scratch(ctx, L);
    rc = rc == FTK_OK ? ftk_ensure_pinned(ctx, L) : rc;
    *dbase = ctx->scratch.as<uint8_t>();
    *hbase = ctx->pinned.as<uint8_t>();
    return rc;
}

// Helpers of one family that ftk_warmup uses too.
// The next image-staging slot, free and at least `bytes` large (ImageStage above); *out stays null when the device cannot address
// pinned host memory (the callers then take their copy paths).  ftk_pyramid.cpp
int ftk_acquire_image_stage(ftk_context *ctx, size_t bytes, ftk_context::ImageStage **out);
int ftk_ensure_match_keys(ftk_context *ctx, size_t count);                      // ftk_match.cpp
int ftk_ensure_brief_pattern(ftk_context *ctx, int32_t n_bits, int32_t half);   // ftk_features.cpp
