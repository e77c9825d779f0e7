// ftk_match_table.cpp — the landmark table of MatchVideoTracker behind the C ABI (include/ftk.h): the table as a
// matcher's reference set, and one frame's matches into the table, over device arrays the caller owns; nothing is copied to the host,
// nothing synchronises and nothing is allocated.
#include "ftk_internal.h"
#include "match_table_plan.h"

static_assert(FTK_MATCH_TABLE_MAX_SLOTS == ftk::kMatchTableMaxSlots && FTK_MATCH_TABLE_MAX_DIM == ftk::kMatchTableMaxDim,
              "include/ftk.h states the limits");
static_assert(FTK_MATCH_TABLE_MAX_SLOTS == FTK_TRANSFORMER_MAX_ROWS && FTK_MATCH_TABLE_MAX_SLOTS == FTK_MATCH_ASSIGNMENT_MAX_ROWS,
              "the table's rows are a matcher's rows: the limits are one number");
static_assert(FTK_MATCH_TABLE_MAX_SLOTS == 4 * FTK_TRACK_TABLE_BLOCK, "four flags per thread of the one scan workgroup");

namespace {

// The plan of a call, or its refusal as the entry's return value.
int plan_call(ftk_context *ctx, const char *who, int32_t n_slots, int32_t rows_cur, int32_t dim, bool aligned16, ftk::MatchTablePlan *plan) {
    ftk::MatchTablePlanInput in{};
    in.n_slots = n_slots;
    in.rows_cur = rows_cur;
    in.dim = dim;
    in.aligned16 = aligned16 ? 1 : 0;
    *plan = ftk::match_table_plan(in);
    switch (plan->refused) {
        case ftk::MatchTableRefusal::None:
            return FTK_OK;
        case ftk::MatchTableRefusal::Slots:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: %d slots outside 1 .. %d", who, n_slots, FTK_MATCH_TABLE_MAX_SLOTS);
        case ftk::MatchTableRefusal::Rows:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: %d current rows outside 1 .. %d", who, rows_cur, FTK_MATCH_TABLE_MAX_SLOTS);
        default:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: descriptor dimension %d outside 1 .. %d", who, dim, FTK_MATCH_TABLE_MAX_DIM);
    }
}

// Two of the call's arrays at one address (null pointers aside).
bool any_equal(const void *const *ptrs, int count) {
    for (int a = 0; a < count; ++a) {
        for (int b = a + 1; b < count; ++b) {
            if (ptrs[a] && ptrs[a] == ptrs[b]) {
                return true;
            }
        }
    }
    return false;
}

ftk::MatchTable table_of(int32_t n_slots, int32_t dim, int64_t *d_ids, float *d_points, float *d_prev_points, float *d_descriptors, uint8_t *d_status,
                         int32_t *d_age, int32_t *d_lost, int32_t *d_n_live, int64_t *d_next_id) {
    ftk::MatchTable m{};
    m.t.ids = reinterpret_cast<long long *>(d_ids);
    m.t.points = d_points;
    m.t.prev_points = d_prev_points;
    m.t.status = d_status;
    m.t.age = d_age;
    m.t.n_live = d_n_live;
    m.t.next_id = reinterpret_cast<long long *>(d_next_id);
    m.t.n = n_slots;
    m.descriptors = d_descriptors;
    m.lost = d_lost;
    m.dim = dim;
    return m;
}

}  // namespace

extern "C" {

int ftk_match_table_workspace_bytes(int32_t n_slots, int32_t rows_cur, int32_t dim, int64_t *bytes) {
    const char *who = "match_table_workspace_bytes";
    return ftk_workspace_bytes<ftk::MatchTablePlan>(who, bytes, [&](ftk::MatchTablePlan *plan) { return plan_call(nullptr, who, n_slots, rows_cur, dim, false, plan); });
}

int ftk_match_table_query_device(ftk_context *ctx, void *stream, int32_t n_slots, int32_t dim, const int64_t *d_ids, const float *d_points,
                                 const float *d_descriptors, float *d_q_uv, float *d_q_desc, int32_t *d_q_slot, int32_t *d_q_count) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "match_table_query_device: null context");
    }
    FTK_LOCK(ctx);
    ftk::MatchTablePlan plan;
    const int rc = plan_call(ctx, "match_table_query_device", n_slots, 1, dim, ftk_aligned(d_descriptors, 16) && ftk_aligned(d_q_desc, 16), &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (!d_ids || !d_points || !d_descriptors || !d_q_uv || !d_q_desc || !d_q_slot || !d_q_count) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "match_table_query_device: null buffer");
    }
    if (!ftk_aligned(d_ids, 8) || !ftk_aligned(d_points, 8) || !ftk_aligned(d_q_uv, 8) || !ftk_aligned(d_descriptors, 4) || !ftk_aligned(d_q_desc, 4) ||
        !ftk_aligned(d_q_slot, 4) || !ftk_aligned(d_q_count, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "match_table_query_device: ids and the (u, v) arrays must be 8-byte aligned, the others 4-byte");
    }
    const void *const ptrs[] = {d_ids, d_points, d_descriptors, d_q_uv, d_q_desc, d_q_slot, d_q_count};
    if (any_equal(ptrs, 7)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "match_table_query_device: no argument may alias another");
    }
    ftk::MatchTableQueryParams p{};
    p.m = table_of(n_slots, dim, const_cast<int64_t *>(d_ids), const_cast<float *>(d_points), nullptr, const_cast<float *>(d_descriptors), nullptr, nullptr,
                   nullptr, nullptr, nullptr);
    p.q_uv = d_q_uv;
    p.q_desc = d_q_desc;
    p.q_slot = d_q_slot;
    p.q_count = d_q_count;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::match_table_query_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

int ftk_match_table_update_device(ftk_context *ctx, void *stream, int32_t n_slots, int32_t dim, int64_t *d_ids, float *d_points, float *d_prev_points,
                                  float *d_descriptors, uint8_t *d_status, int32_t *d_age, int32_t *d_lost, int32_t *d_n_live, int64_t *d_next_id,
                                  const int32_t *d_q_slot, const int32_t *d_q_count, const int32_t *d_match_index, const uint8_t *d_match_status,
                                  const float *d_cur_uv, const float *d_cur_desc, int32_t rows_cur, const int32_t *d_cur_count, int32_t max_lost,
                                  void *d_workspace, int32_t *d_cur_slot) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "match_table_update_device: null context");
    }
    FTK_LOCK(ctx);
    ftk::MatchTablePlan plan;
    const int rc = plan_call(ctx, "match_table_update_device", n_slots, rows_cur, dim, ftk_aligned(d_descriptors, 16) && ftk_aligned(d_cur_desc, 16), &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (max_lost < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "match_table_update_device: max_lost %d must be >= 0", max_lost);
    }
    if (!d_ids || !d_points || !d_prev_points || !d_descriptors || !d_status || !d_age || !d_lost || !d_n_live || !d_next_id || !d_q_slot || !d_q_count ||
        !d_match_index || !d_match_status || !d_cur_uv || !d_cur_desc || !d_workspace) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "match_table_update_device: null buffer");
    }
    if (!ftk_aligned(d_workspace, 16) || !ftk_aligned(d_ids, 8) || !ftk_aligned(d_next_id, 8) || !ftk_aligned(d_points, 8) || !ftk_aligned(d_prev_points, 8) ||
        !ftk_aligned(d_cur_uv, 8) || !ftk_aligned(d_descriptors, 4) || !ftk_aligned(d_cur_desc, 4) || !ftk_aligned(d_age, 4) || !ftk_aligned(d_lost, 4) ||
        !ftk_aligned(d_n_live, 4) || !ftk_aligned(d_q_slot, 4) || !ftk_aligned(d_q_count, 4) || !ftk_aligned(d_match_index, 4) || !ftk_aligned(d_cur_count, 4) ||
        !ftk_aligned(d_cur_slot, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT,
                        "match_table_update_device: the workspace must be 16-byte aligned, the int64 and (u, v) arrays 8-byte, the others 4-byte");
    }
    const void *const ptrs[] = {d_ids, d_points, d_prev_points, d_descriptors, d_status, d_age, d_lost, d_n_live, d_next_id, d_q_slot, d_q_count,
                                d_match_index, d_match_status, d_cur_uv, d_cur_desc, d_cur_count, d_workspace, d_cur_slot};
    if (any_equal(ptrs, 18)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "match_table_update_device: no argument may alias another");
    }
    ftk::MatchTableUpdateParams p{};
    p.m = table_of(n_slots, dim, d_ids, d_points, d_prev_points, d_descriptors, d_status, d_age, d_lost, d_n_live, d_next_id);
    p.q_slot = d_q_slot;
    p.q_count = d_q_count;
    p.match_index = d_match_index;
    p.match_status = d_match_status;
    p.cur_uv = d_cur_uv;
    p.cur_desc = d_cur_desc;
    p.cur_count = d_cur_count;
    p.rows_cur = rows_cur;
    p.max_lost = max_lost;
    p.cur_slot = d_cur_slot ? d_cur_slot : plan.cur_slot.in(d_workspace);
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::match_table_update_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
