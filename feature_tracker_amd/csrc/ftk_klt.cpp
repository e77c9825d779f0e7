// ftk_klt.cpp — the trackers' entry points of the C ABI (include/ftk.h): ftk_klt_track_device and its host-buffer wrapper.
//
// One call, in the order it runs: argument checks -> tail class (klt_tail_class) -> launch plan (klt_plan.h: a pure function) ->
// this launch's number for the tail report -> the large-patch batches (klt_launch_spilled) OR the launch order (klt_sched_prepare)
// -> launch.  Reading the world — the context, the FTK_KLT_* switches, the device's tail words — happens here, never in the plan
// nor in the two state machines that decide tail class and launch order (klt_sched.h: pure step functions).
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ftk_device.h"
#include "ftk_internal.h"
#include "klt_plan.h"

namespace {

int klt_check_call(ftk_context *ctx, int model, const ftk_klt_options *opt, const ftk_pyramid *ref, const ftk_pyramid *cur) {
    if (!opt || !ref || !cur) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "klt: null options or pyramid");
    }
    if (model < FTK_MODEL_BASIC || model > FTK_MODEL_LSSD) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "klt: unknown model %d", model);
    }
    if (opt->method < FTK_METHOD_INVERSE || opt->method > FTK_METHOD_NEON) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "klt: unknown method %d", opt->method);
    }
    if (ref->n_levels != cur->n_levels) {
        // OpticalFlow::TrackFeatures returns false here (optical_flow.cpp:9); callers above the ABI handle it
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "klt: pyramid level mismatch (%d vs %d)", ref->n_levels, cur->n_levels);
    }
    if (ref->n_levels < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "klt: empty pyramid");
    }
    if (ref->device != ctx->device || cur->device != ctx->device) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "klt: pyramid lives on another device");
    }
    // The reference takes any int32 half size (optical_flow.h:24-25).  Here: up to 1023 (a 2047 x 2047 patch; pixel indices stay
    // below 2^23 for the 24-bit multiplier); patches beyond a workgroup's LDS run the large-patch form below.
    if (opt->half_rows < 0 || opt->half_cols < 0 || opt->half_rows > 1023 || opt->half_cols > 1023) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "klt: half patch size (%d, %d) outside [0, 1023]", opt->half_rows, opt->half_cols);
    }
    return FTK_OK;
}

// An FTK_KLT_* count override: "atoi, clamp 1..4", or kKltNotSet.
int klt_count_override(const char *env) {
    if (!env) {
        return ftk::kKltNotSet;
    }
    const int v = atoi(env);
    return v < 1 ? 1 : (v > 4 ? 4 : v);
}

// Tail class of this variant's next launch (the wave policy's second axis, klt_plan.cpp), from the word its kernels report into
// (klt_sched.h klt_tail_class_step).  FTK_KLT_TAIL_CLASS pins the class (the sweep and the policy test).
int klt_tail_class(ftk_context *ctx, int model, int method) {
    int long_tail = 0;
    if (ctx->tail_host) {
        long_tail = ftk::klt_tail_class_step(ctx->tail, model, method, ctx->tail_host.as<volatile uint32_t>()[model * 3 + ftk::klt_method_class(method)]);
    }
    if (const char *env = FTK_ENV(ctx, klt_tail_class)) {
        long_tail = atoi(env) != 0 ? 1 : 0;  // experiment override
    }
    return long_tail;
}

// The call's own fields of the argument block, then the plan (geometry and launch shape).
int klt_plan_call(ftk_context *ctx, int model, const ftk_klt_options *opt, const ftk_pyramid *ref, const ftk_pyramid *cur, int32_t n, const float *prior,
                  int consider_luminance, int single_level, int long_tail, ftk::KltParams *out, ftk::KltPlan *plan) {
    ftk::KltParams &p = *out;
    memset(&p, 0, sizeof(p));  // (every pointer null: list order, nothing recorded, unless a later step installs it)
    ftk::KltPlanInput in = {};
    p.n_levels = single_level ? 1 : ref->n_levels;
    p.single_level = single_level ? 1 : 0;
    p.scale_recip = (p.n_levels - 1 <= 30) ? 1 : 0;  // (always, while FTK_MAX_LEVELS <= 31: the kernels take it from here, not from that)
    for (int i = 0; i < p.n_levels; ++i) {
        p.ref[i] = ref->levels[i];
        p.cur[i] = cur->levels[i];
        in.max_extent = std::max({in.max_extent, p.ref[i].rows, p.ref[i].cols, p.cur[i].rows, p.cur[i].cols});
    }
    p.n = n;
    p.n_track = ((uint32_t)n < opt->max_track_points) ? (uint32_t)n : opt->max_track_points;
    p.max_iteration = opt->max_iteration;
    p.max_large_step = opt->max_tolerance_large_step;
    p.converge = opt->max_converge_step;
    static const float identity[4] = {1.0f, 0.0f, 0.0f, 1.0f};
    const float *pr = prior ? prior : identity;
    for (int i = 0; i < 4; ++i) {
        p.prior[i] = pr[i];
    }
    p.consider_luminance = consider_luminance ? 1 : 0;
    in.model = model;
    in.method = opt->method;
    in.half_rows = opt->half_rows;
    in.half_cols = opt->half_cols;
    in.n = n;
    in.consider_luminance = p.consider_luminance;
    in.tree = ctx->reduction == FTK_REDUCTION_TREE ? 1 : 0;
    in.long_tail = long_tail;
    in.waves = klt_count_override(FTK_ENV(ctx, klt_waves));
    in.group = klt_count_override(FTK_ENV(ctx, klt_group));
    in.lssd_chunked = FTK_ENV(ctx, lssd_chunked) ? atoi(FTK_ENV(ctx, lssd_chunked)) : ftk::kKltNotSet;
    in.spill = FTK_ENV(ctx, klt_spill) ? atoi(FTK_ENV(ctx, klt_spill)) : ftk::kKltNotSet;
    size_t spill_floats = 0;
    switch (ftk::klt_plan(in, &p, plan, &spill_floats)) {
        case ftk::kKltPlanUnknownVariant: return ftk_fail(ctx, FTK_E_UNSUPPORTED, "klt: unknown variant (model %d, method %d)", model, opt->method);
        case ftk::kKltPlanSpillTooLarge:
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "klt: patch %dx%d needs %zu floats of device memory per feature", p.patch_rows, p.patch_cols, spill_floats);
        default: return FTK_OK;
    }
}

// This launch's number, for the report of its longest feature (the tail words are allocated on a context's first tracker call
// outside a stream capture; until then, and when that fails, the launches carry no tail words).
void klt_tail_number(ftk_context *ctx, int model, int method, ftk::KltParams &p) {
    if (!ctx->tail_host && !ftk_stream_capturing(ctx->stream)) {
        if (ctx->tail_host.reserve(ctx->stream, 64, 0, 1) == hipSuccess && ctx->tail_dev.reserve(ctx->stream, 64, 0, 1) == hipSuccess) {
            memset(ctx->tail_host.get(), 0, 64);
            (void)hipMemsetAsync(ctx->tail_dev.get(), 0, 64, ctx->stream);
        } else {
            (void)hipGetLastError();
            ctx->tail_host.release();
            ctx->tail_dev.release();
        }
    }
    if (ctx->tail_host && ctx->tail_dev) {
        bool wipe_device_word = false;
        p.tail_call = ftk::klt_tail_next_call(ctx->tail, model, method, &wipe_device_word);
        if (wipe_device_word) {
            (void)hipMemsetAsync(ctx->tail_dev.get(), 0, 64, ctx->stream);
        }
        const int word = model * 3 + ftk::klt_method_class(method);
        p.tail_dev = ctx->tail_dev.as<uint32_t>() + word;    // a word per variant
        p.tail_host = ctx->tail_host.as<uint32_t>() + word;  // (pinned host memory is device-visible under the same address)
    }
}

// Large patches: a slice of device memory per launch slot.  All features at once while that stays within a budget (4 GB;
// FTK_KLT_SPILL_BUDGET_MB), otherwise in batches of consecutive features — a feature's result does not depend on the others.
int klt_launch_spilled(ftk_context *ctx, int model, int method, ftk::KltParams &p, const ftk::KltPlan &plan) {
    const int32_t n = p.n;
    const size_t per = sizeof(float) * (size_t)p.spill_stride_floats;
    size_t budget = (size_t)4096 << 20;
    if (const char *env = FTK_ENV(ctx, klt_spill_budget_mb)) {
        budget = (size_t)(atoll(env) > 0 ? atoll(env) : 1) << 20;
    }
    size_t batch = budget / per;
    batch = batch < 1 ? 1 : (batch > (size_t)n ? (size_t)n : batch);
    // the slices would have to grow: a release, an allocation (and a synchronisation) that a stream capture cannot contain
    if (batch * per > ctx->klt_spill.bytes() && ftk_stream_capturing(ctx->stream)) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "klt_track_device: a %d x %d patch needs %zu MB of device memory for its per-feature slices, which cannot be "
                        "allocated while the stream is being captured: make one such call before the capture (the buffer is kept)", p.patch_rows, p.patch_cols,
                        (batch * per) >> 20);
    }
    const int rc_buf = ftk_ensure_device_buffer(ctx, ctx->klt_spill, batch * per);
    if (rc_buf != FTK_OK) {
        return rc_buf;
    }
    p.spill_base = ctx->klt_spill.as<float>();
    ftk::klt_sched_reset(ctx->sched);  // no launch order for these calls; a later ordinary call starts its history over
    for (size_t b0 = 0; b0 < (size_t)n; b0 += batch) {
        const size_t nb = (size_t)n - b0 < batch ? (size_t)n - b0 : batch;
        ftk::KltParams q = p;
        q.n = (int32_t)nb;
        q.ref_uv = p.ref_uv + 2 * b0;
        q.cur_uv_in = p.cur_uv_in + 2 * b0;
        q.cur_uv_out = p.cur_uv_out + 2 * b0;
        q.status_in = p.status_in + b0;
        q.status_out = p.status_out + b0;
        q.iters = p.iters ? p.iters + b0 : nullptr;
        q.n_track = (size_t)p.n_track > b0 ? (uint32_t)((size_t)p.n_track - b0 < nb ? (size_t)p.n_track - b0 : nb) : 0u;  // kMaxTrackPointsNumber is a cap on the whole list
        ftk::KltPlan batch_plan = plan;
        batch_plan.grid = (unsigned)nb;  // one workgroup per feature in this form
        const hipError_t e = ftk::klt_launch(batch_plan, model, method, q, ctx->stream);
        if (e != hipSuccess) {
            return ftk_fail(ctx, e == hipErrorOutOfMemory ? FTK_E_OUT_OF_MEMORY : FTK_E_HIP, "klt launch (large patch) failed: %s", hipGetErrorString(e));
        }
    }
    return FTK_OK;
}

// Every buffer of the launch order for `cap` features: the double-buffered counts and orders, a claim word per launch slot, a
// predicted count per feature and (once) the grid buffer (klt_sched.h: two position tables, flags, order workspace).
int klt_sched_grow(ftk_context *ctx, size_t cap) {
    FTK_HIP(ctx, ctx->sched_claim.reserve(ctx->stream, sizeof(uint32_t) * cap, 0, 1));
    FTK_HIP(ctx, hipMemsetAsync(ctx->sched_claim.get(), 0, sizeof(uint32_t) * cap, ctx->stream));
    FTK_HIP(ctx, ctx->sched_pred.reserve(ctx->stream, cap, 0, 1));
    bool new_grid = false;
    FTK_HIP(ctx, ctx->sched_grid.reserve(ctx->stream, sizeof(uint32_t) * ftk::kSchedGridWords, 0, 1, &new_grid));
    if (new_grid) {
        FTK_HIP(ctx, hipMemsetAsync(ctx->sched_grid.get(), 0, sizeof(uint32_t) * ftk::kSchedTableWords, ctx->stream));
    }
    for (int k = 0; k < 2; ++k) {
        FTK_HIP(ctx, ctx->sched_iters[k].reserve(ctx->stream, sizeof(uint32_t) * cap, 0, 1));
        FTK_HIP(ctx, ctx->sched_order[k].reserve(ctx->stream, sizeof(int32_t) * cap, 0, 1));
        // never-written entries must still be valid feature ids (0) and valid counts, whatever happens to a launch
        FTK_HIP(ctx, hipMemsetAsync(ctx->sched_iters[k].get(), 0, sizeof(uint32_t) * cap, ctx->stream));
        FTK_HIP(ctx, hipMemsetAsync(ctx->sched_order[k].get(), 0, sizeof(int32_t) * cap, ctx->stream));
    }
    return FTK_OK;
}

// The two diagnostics of the launch order, each into the file its switch names (they synchronise the stream).
int klt_sched_dump(ftk_context *ctx, const ftk::KltSchedStep &step, int32_t n) {
    const char *dump = FTK_ENV(ctx, klt_swap_dump);  // how many trades the PREVIOUS launch of this context made
    if (dump && step.trades && step.sched_call > 5u) {
        std::vector<uint32_t> h((size_t)n);
        FTK_HIP(ctx, hipMemcpyAsync(h.data(), ctx->sched_claim.as<uint32_t>(), sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        size_t trades = 0, own = 0;
        for (uint32_t w : h) {
            if (ftk::sched_claim_call(w) == ftk::sched_claim_tag(step.sched_call - 1u)) {
                (ftk::sched_claim_code(w) == ftk::kSchedSelf ? own : trades) += 1;
            }
        }
        if (FILE *f = fopen(dump, "w")) {
            fprintf(f, "%zu %zu\n", trades, own);
            fclose(f);
        }
    }
    dump = FTK_ENV(ctx, klt_sched_dump);  // the index-keyed permutation in use and the counts it came from (still in the buffer this call will overwrite)
    if (dump && step.order == ftk::KltOrder::Index) {
        std::vector<int32_t> h((size_t)n * 2);
        FTK_HIP(ctx, hipMemcpyAsync(h.data(), ctx->sched_order[step.order_buf].as<int32_t>(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        FTK_HIP(ctx, hipMemcpyAsync(h.data() + n, ctx->sched_iters[step.iters_buf].as<uint32_t>(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (FILE *f = fopen(dump, "wb")) {
            fwrite(h.data(), sizeof(int32_t), h.size(), f);
            fclose(f);
        }
    }
    return FTK_OK;
}

// Launch order of this call (klt_sched.h klt_sched_step decides): inputs, step, act.
int klt_sched_prepare(ftk_context *ctx, int model, int32_t n, int long_tail, ftk::KltParams &p) {
    ftk::KltSchedInput in = {};
    in.n = n;
    in.n_track = p.n_track;
    in.model = model;
    in.waves_per_feature = p.waves_per_feature;
    in.long_tail = long_tail;
    in.sched = FTK_ENV(ctx, klt_sched) ? atoi(FTK_ENV(ctx, klt_sched)) : ftk::kKltNotSet;
    // (a negative threshold was always read as an unsigned one: above every feature count)
    in.sched_min = FTK_ENV(ctx, klt_sched_min) ? (atoi(FTK_ENV(ctx, klt_sched_min)) < 0 ? INT32_MAX : atoi(FTK_ENV(ctx, klt_sched_min))) : ftk::kKltNotSet;
    if (!ftk::klt_sched_applies(in)) {
        return FTK_OK;  // list order, and nothing else to ask
    }
    in.capturing = ftk_stream_capturing(ctx->stream);
    const char *ref_lo = reinterpret_cast<const char *>(p.ref_uv), *out_lo = reinterpret_cast<const char *>(p.cur_uv_out);
    const size_t uv_span = sizeof(float) * 2 * (size_t)n;
    in.ref_untouched = ref_lo + uv_span <= out_lo || out_lo + uv_span <= ref_lo;
    in.have_grid = (bool)ctx->sched_grid;
    in.have_claim = (bool)ctx->sched_claim;
    in.have_pred = (bool)ctx->sched_pred;

    ftk::KltSchedState next = ctx->sched;  // (installed once the buffers it counts on exist)
    const ftk::KltSchedStep step = ftk::klt_sched_step(next, in);

    if (step.grow_to != 0) {
        const int rc = klt_sched_grow(ctx, step.grow_to);
        if (rc != FTK_OK) {
            ctx->sched.capacity = 0;
            ftk::klt_sched_reset(ctx->sched);
            return rc;
        }
    }
    if (step.wipe_claims_and_grid) {
        FTK_HIP(ctx, hipMemsetAsync(ctx->sched_claim.get(), 0, sizeof(uint32_t) * next.capacity, ctx->stream));
        FTK_HIP(ctx, hipMemsetAsync(ctx->sched_grid.get(), 0, sizeof(uint32_t) * ftk::kSchedTableWords, ctx->stream));
    }
    ctx->sched = next;
    uint32_t *grid = ctx->sched_grid.as<uint32_t>();
    if (step.recording) {
        p.sched_grid = grid;
        p.sched_call = step.sched_call;
    }
    if (step.trades) {
        p.sched_flags = grid + ftk::kSchedFlagsAt;
        p.sched_claim = ctx->sched_claim.as<uint32_t>();
    }
    p.sched_iters = ctx->sched_iters[step.iters_buf].as<uint32_t>();
    if (step.sort_from >= 0) {
        p.sort_iters = ctx->sched_iters[step.sort_from].as<uint32_t>();
        p.sort_order_out = ctx->sched_order[step.sort_from].as<int32_t>();
        p.sort_ref_uv = step.sort_reads_ref_uv ? p.ref_uv : nullptr;
    }
    if (step.order != ftk::KltOrder::None) {
        int32_t *order = ctx->sched_order[step.order_buf].as<int32_t>();
        if (step.order == ftk::KltOrder::Position) {
            FTK_HIP(ctx, ftk::klt_position_order_launch(p.ref_uv, n, grid + ftk::sched_table_at(step.sched_call - 1u), step.sched_call - 1u,
                                                        ctx->sched_pred.as<uint8_t>(), grid + ftk::kSchedTableWords, order, ctx->stream));
        }
        p.order = order;
    }
    return klt_sched_dump(ctx, step, n);
}

}  // namespace

void ftk_default_klt_options(ftk_klt_options *opt) {
    if (!opt) {
        return;
    }
    opt->max_track_points = 500;
    opt->max_iteration = 15;
    opt->max_tolerance_large_step = 3;
    opt->half_rows = 6;
    opt->half_cols = 6;
    opt->max_converge_step = 4e-2f;
    opt->method = FTK_METHOD_FAST;
}

int ftk_klt_track_device(ftk_context *ctx, int model, const ftk_klt_options *opt, const ftk_pyramid *ref, const ftk_pyramid *cur,
                         const float *d_ref_uv, const float *d_cur_uv_in, float *d_cur_uv_out, const uint8_t *d_status_in,
                         uint8_t *d_status_out, int32_t n, const float *prior, int consider_luminance, int single_level, uint32_t *d_iters) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "klt_track_device: null context");
    }
    FTK_LOCK(ctx);
    if (n < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "klt_track_device: negative feature count");
    }
    if (n == 0) {
        return FTK_OK;
    }
    if (!d_ref_uv || !d_cur_uv_in || !d_cur_uv_out || !d_status_in || !d_status_out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "klt_track_device: null buffer");
    }
    // The kernels read and write a feature's (u, v) as ONE 8-byte access (include/ftk.h: "8-byte aligned"): a pair array at an odd
    // float offset — legal through round 3 — is refused here instead of becoming misaligned 64-bit accesses on the device.
    if (((reinterpret_cast<uintptr_t>(d_ref_uv) | reinterpret_cast<uintptr_t>(d_cur_uv_in) | reinterpret_cast<uintptr_t>(d_cur_uv_out)) & 7u) != 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "klt_track_device: the (u, v) arrays must be 8-byte aligned (ref %p, in %p, out %p)", (const void *)d_ref_uv,
                        (const void *)d_cur_uv_in, (const void *)d_cur_uv_out);
    }
    int rc = klt_check_call(ctx, model, opt, ref, cur);
    if (rc != FTK_OK) {
        return rc;
    }
    const int long_tail = klt_tail_class(ctx, model, opt->method);
    ftk::KltParams p;
    ftk::KltPlan plan;
    rc = klt_plan_call(ctx, model, opt, ref, cur, n, prior, consider_luminance, single_level, long_tail, &p, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    klt_tail_number(ctx, model, opt->method, p);
    p.ref_uv = d_ref_uv;
    p.cur_uv_in = d_cur_uv_in;
    p.cur_uv_out = d_cur_uv_out;
    p.status_in = d_status_in;
    p.status_out = d_status_out;
    p.iters = d_iters;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    if (plan.form == ftk::KltForm::GenericSpill) {
        return klt_launch_spilled(ctx, model, opt->method, p, plan);
    }
    rc = klt_sched_prepare(ctx, model, n, long_tail, p);
    if (rc != FTK_OK) {
        return rc;
    }
    const hipError_t launch_rc = ftk::klt_launch(plan, model, opt->method, p, ctx->stream);
    if (launch_rc != hipSuccess) {
        // The launch-order state advanced above assumed this launch would write its iteration counts and (from the second call
        // on) a permutation: it did neither, so the history starts over — the next call must not install an order nobody wrote.
        ftk::klt_sched_reset(ctx->sched);
        return ftk_fail(ctx, launch_rc == hipErrorOutOfMemory ? FTK_E_OUT_OF_MEMORY : FTK_E_HIP, "klt launch failed: %s", hipGetErrorString(launch_rc));
    }
    return FTK_OK;
}

int ftk_klt_track(ftk_context *ctx, int model, const ftk_klt_options *opt, const ftk_pyramid *ref, const ftk_pyramid *cur, const float *ref_uv,
                  float *cur_uv, uint8_t *status, int32_t n, const float *prior, int consider_luminance, int single_level, uint32_t *iters) {
    FTK_TRACE_SCOPE("ftk_klt_track");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "klt_track: null context");
    }
    FTK_LOCK(ctx);
    if (n < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "klt_track: negative feature count");
    }
    if (n == 0) {
        return FTK_OK;
    }
    if (!ref_uv || !cur_uv || !status) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "klt_track: null buffer");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    // One contiguous block [ref_uv | cur_uv | status | iters], mirrored in pinned host memory:
    // a single H2D of (ref_uv, cur_uv, status) and a single D2H of (cur_uv, status, iters) per call.
    ftk_layout L;
    const auto s_ref = L.take<float>(2 * (size_t)n), s_cur = L.take<float>(2 * (size_t)n);
    const auto s_st = L.take<uint8_t>((size_t)n);
    const auto s_it = L.take<uint32_t>((size_t)n);
    uint8_t *dbase = nullptr, *hbase = nullptr;
    int rc = ftk_ensure_mirror(ctx, L, &dbase, &hbase);
    if (rc != FTK_OK) {
        return rc;
    }
    memcpy(s_ref.in(hbase), ref_uv, s_ref.size_bytes());
    memcpy(s_cur.in(hbase), cur_uv, s_cur.size_bytes());
    memcpy(s_st.in(hbase), status, s_st.size_bytes());
    // Small calls (the reference's callers track a few hundred features) are dominated by the two staging copies and
    // their queue latency, not by bytes: the kernel then reads (ref_uv, cur_uv, status) from and writes its 9 B per
    // feature straight into the pinned host block over PCIe — no H2D / D2H at all (2 000 features: 89 -> ~60 us per
    // call).  Larger calls keep the bulk copies.
    void *mapped = nullptr;
    const bool zero_copy = n <= 16384 && hipHostGetDevicePointer(&mapped, ctx->pinned.get(), 0) == hipSuccess && mapped != nullptr;
    uint8_t *base = zero_copy ? static_cast<uint8_t *>(mapped) : dbase;  // what the device entry works on
    if (!zero_copy) {
        FTK_HIP(ctx, hipMemcpyAsync(s_ref.in(dbase), s_ref.in(hbase), L.span_bytes(s_ref, s_st), hipMemcpyHostToDevice, ctx->stream));
    }
    rc = ftk_klt_track_device(ctx, model, opt, ref, cur, s_ref.in(base), s_cur.in(base), s_cur.in(base), s_st.in(base), s_st.in(base), n, prior, consider_luminance,
                              single_level, iters ? s_it.in(base) : nullptr);
    if (rc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    if (!zero_copy) {
        FTK_HIP(ctx, hipMemcpyAsync(s_cur.in(hbase), s_cur.in(dbase), iters ? L.span_bytes(s_cur, s_it) : L.span_bytes(s_cur, s_st), hipMemcpyDeviceToHost, ctx->stream));
    }
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(cur_uv, s_cur.in(hbase), s_cur.size_bytes());
    memcpy(status, s_st.in(hbase), s_st.size_bytes());
    if (iters) {
        memcpy(iters, s_it.in(hbase), s_it.size_bytes());
    }
    return FTK_OK;
}

int ftk_extract_extend_patch(ftk_context *ctx, const ftk_pyramid *ref, int32_t level, float u, float v, int32_t ex_rows, int32_t ex_cols,
                             float *ex_patch, uint8_t *valid, uint32_t *valid_count) {
    FTK_TRACE_SCOPE("ftk_extract_extend_patch");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "extract_extend_patch: null context");
    }
    FTK_LOCK(ctx);
    if (!ref || level < 0 || level >= ref->n_levels || ex_rows <= 0 || ex_cols <= 0 || !ex_patch || !valid || !valid_count) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "extract_extend_patch: bad arguments");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ex_rows * ex_cols;
    ftk_layout L;
    const auto s_patch = L.take<float>(n);
    const auto s_valid = L.take<uint8_t>(n);
    const auto s_count = L.take<uint32_t>(1);
    int rc = ftk_ensure_scratch(ctx, L);
    if (rc != FTK_OK) {
        return rc;
    }
    void *base = ctx->scratch.get();
    float *d_patch = s_patch.in(base);
    uint8_t *d_valid = s_valid.in(base);
    uint32_t *d_count = s_count.in(base);
    FTK_HIP(ctx, ftk::extract_patch_launch(ref->levels[level], u, v, ex_rows, ex_cols, d_patch, d_valid, d_count, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(ex_patch, d_patch, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(valid, d_valid, n, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(valid_count, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}
