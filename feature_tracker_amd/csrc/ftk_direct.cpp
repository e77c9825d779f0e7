// ftk_direct.cpp — the direct method (photometric pose tracking) of the C ABI (include/ftk.h).
#include <string.h>

#include <algorithm>
#include <vector>

#include "ftk_internal.h"
#include "match_plan.h"

namespace {

int env_int(const char *v) { return v ? atoi(v) : ftk::kPlanNotSet; }  // an FTK_* switch as a plan input

// The kernels' problem table from the caller's problems (checked here); *max_features: tracked features of the largest problem.
int direct_problem_table(ftk_context *ctx, const ftk_direct_options *opt, const ftk_direct_problem *problems, int32_t n_problems,
                         std::vector<ftk::DirectProblem> *table, uint32_t *max_features, int32_t *n_levels) {
    table->resize((size_t)n_problems);
    for (int32_t k = 0; k < n_problems; ++k) {
        const ftk_direct_problem &in = problems[k];
        if (!in.ref || !in.cur || in.n < 0 || (in.n > 0 && (!in.d_p_c_in_ref || !in.d_ref_uv || !in.d_cur_uv || !in.d_status)) || !in.d_pose) {
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "direct_track: problem %d has a null buffer", k);
        }
        if (in.ref->n_levels != in.cur->n_levels || in.ref->n_levels < 1) {
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "direct_track: problem %d pyramid level mismatch (%d vs %d)", k, in.ref->n_levels, in.cur->n_levels);
        }
        if (k == 0) {
            *n_levels = in.ref->n_levels;
        } else if (in.ref->n_levels != *n_levels) {
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "direct_track: all problems of a batch must share the pyramid depth");
        }
        if (in.ref->device != ctx->device || in.cur->device != ctx->device) {
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "direct_track: pyramid lives on another device");
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
        const int rc = ftk_ensure_device_buffer(ctx, ctx->direct_feat, plan.feat_bytes * n_problems);
        if (rc != FTK_OK) {
            return rc;
        }
        for (size_t k = 0; k < n_problems; ++k) {
            table[k].feat = reinterpret_cast<float4 *>(ctx->direct_feat.as<uint8_t>() + plan.feat_bytes * k);
        }
    }
    const size_t table_bytes = sizeof(ftk::DirectProblem) * n_problems;
    FTK_HIP(ctx, ctx->direct_table.reserve(ctx->stream, table_bytes, 0, 4096));
    // pageable host -> device copy: synchronous with respect to the host buffer, so `table` may go out of scope
    FTK_HIP(ctx, hipMemcpyAsync(ctx->direct_table.get(), table.data(), table_bytes, hipMemcpyHostToDevice, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

// ftk_direct_track_batch_device; spread_allowed = false: the re-run of a poisoned spread launch on one workgroup per problem.
int direct_track_batch(ftk_context *ctx, const ftk_direct_options *opt, const ftk_direct_problem *problems, int32_t n_problems, bool spread_allowed) {
    if (!opt || n_problems < 0 || (n_problems > 0 && !problems)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "direct_track: null options / problems");
    }
    if (n_problems == 0) {
        return FTK_OK;
    }
    if (opt->half_rows < 0 || opt->half_cols < 0 || opt->half_rows > 63 || opt->half_cols > 63) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "direct_track: half patch size (%d, %d) outside [0, 63]", opt->half_rows, opt->half_cols);
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
                               spread_allowed, resident_known ? ctx->direct_spread_resident : ftk::kPlanNotSet, ftk::kPlanNotSet, ctx->direct_spread.bytes(),
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
        in.capturing = ftk_stream_capturing(ctx->stream);
        plan = ftk::direct_plan(in);
    }
    ctx->direct_spread_launched = 0;
    if (plan.producers > 0) {
        rc = ftk_ensure_device_buffer(ctx, ctx->direct_spread, plan.ws_stride * (size_t)n_problems);
        if (rc != FTK_OK) {
            return rc;
        }
        for (int32_t k = 0; k < n_problems; ++k) {  // header + chunk flags of every problem: zero before the launch
            FTK_HIP(ctx, hipMemsetAsync(ctx->direct_spread.as<uint8_t>() + plan.ws_stride * (size_t)k, 0, plan.clear_bytes, ctx->stream));
        }
        ctx->direct_spread_launched = n_problems;
    }
    const ftk::DirectParams p = {ctx->direct_table.as<const ftk::DirectProblem>(), in.tree, n_levels, opt->max_track_points, opt->max_iteration,
                                 opt->half_rows, opt->half_cols, in.patch_rows, in.patch_cols, opt->max_converge_step, opt->method, plan.producers,
                                 plan.producers > 0 ? ctx->direct_spread.as<uint32_t>() : nullptr, (uint32_t)(plan.ws_stride / sizeof(uint32_t)),
                                 plan.poison};
    FTK_HIP(ctx, ftk::direct_track_launch(plan, p, ctx->stream));
    return FTK_OK;
}

}  // namespace

extern "C" {

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

int ftk_direct_track_batch_device(ftk_context *ctx, const ftk_direct_options *opt, const ftk_direct_problem *problems, int32_t n_problems) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "direct_track: null context");
    }
    FTK_LOCK(ctx);
    return direct_track_batch(ctx, opt, problems, n_problems, true);
}

int ftk_direct_track(ftk_context *ctx, const ftk_direct_options *opt, const ftk_pyramid *ref, const ftk_pyramid *cur, const float *K,
                     const float *p_c_in_ref, const float *ref_uv, float *cur_uv, int32_t n, float *q_rc_wxyz, float *p_rc, uint8_t *status,
                     int status_valid, uint32_t *iterations) {
    FTK_TRACE_SCOPE("ftk_direct_track");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "direct_track: null context");
    }
    FTK_LOCK(ctx);
    if (n < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "direct_track: negative feature count");
    }
    if (n == 0) {
        return FTK_OK;  // the class returns false for an empty ref_pixel_uv (:38); nothing to compute here
    }
    if (!opt || !ref || !cur || !K || !p_c_in_ref || !ref_uv || !cur_uv || !q_rc_wxyz || !p_rc || !status) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "direct_track: null argument");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    ftk_layout L;
    const auto s_pts = L.take<float>(3 * (size_t)n);
    const auto s_ref = L.take<float>(2 * (size_t)n), s_cur = L.take<float>(2 * (size_t)n);
    const auto s_st = L.take<uint8_t>((size_t)n);
    const auto s_pose = L.take<float>(7);
    const auto s_it = L.take<uint32_t>(1);
    int rc = ftk_ensure_scratch(ctx, L);
    if (rc != FTK_OK) {
        return rc;
    }
    void *base = ctx->scratch.get();
    float *d_pts = s_pts.in(base), *d_ref = s_ref.in(base), *d_cur = s_cur.in(base), *d_pose = s_pose.in(base);
    uint8_t *d_st = s_st.in(base);
    uint32_t *d_it = s_it.in(base);
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
        FTK_HIP(ctx, hipMemcpyAsync(&poisoned, ctx->direct_spread.as<uint32_t>() + 1, sizeof(poisoned), hipMemcpyDeviceToHost, ctx->stream));
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

}  // extern "C"
