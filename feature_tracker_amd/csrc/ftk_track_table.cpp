// ftk_track_table.cpp — masked Harris detection on the device and the track table of KltVideoTracker behind the C ABI (include/ftk.h,
// DESIGN.md 5.19): everything stays in device memory, nothing is copied to the host and nothing synchronises.
#include "ftk_internal.h"
#include "track_table_plan.h"

static_assert(FTK_HARRIS_DEVICE_MAX_SURVIVORS == ftk::kHarrisDeviceMaxSurvivors && FTK_TRACK_TABLE_MAX_SLOTS == ftk::kTrackTableMaxSlots &&
                  FTK_HARRIS_RANK_TILE == ftk::kHarrisRankTile && FTK_TRACK_TABLE_BLOCK == ftk::kTrackRetireBlock,
              "include/ftk.h states the limits");

namespace {

bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// The plan of a call, or its refusal as the entry's return value.
int plan_call(ftk_context *ctx, const char *who, const ftk_pyramid *image, int32_t level, int32_t min_distance, int32_t n_slots, int32_t n_occupied,
              ftk::TrackTablePlan *plan) {
    if (!image || level < 0 || level >= image->n_levels) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: bad image / level", who);
    }
    ftk::TrackTablePlanInput in{};
    in.rows = image->levels[level].rows;
    in.cols = image->levels[level].cols;
    in.min_distance = min_distance;
    in.n_slots = n_slots;
    in.n_occupied = n_occupied;
    *plan = ftk::track_table_plan(in);
    switch (plan->refused) {
        case ftk::TrackTableRefusal::None:
            return FTK_OK;
        case ftk::TrackTableRefusal::Survivors:
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: a %d x %d image at min_distance %d can hold more than %d corners: raise min_distance", who, in.rows,
                            in.cols, min_distance, FTK_HARRIS_DEVICE_MAX_SURVIVORS);
        case ftk::TrackTableRefusal::Slots:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: %d slots outside 1 .. %d", who, n_slots, FTK_TRACK_TABLE_MAX_SLOTS);
        default:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: bad sizes (%d x %d, %d occupied points)", who, in.rows, in.cols, n_occupied);
    }
}

// Masked detection up to the survivor list (plan.capacity > 0); *list and *count are in the context's scratch block and hold until its next use.
int detect_survivors(ftk_context *ctx, const ftk::TrackTablePlan &plan, const DevImage &img, int32_t min_distance, float min_response,
                     ftk::HarrisOccupied occupied, unsigned long long **list, unsigned **count) {
    const size_t px = (size_t)img.rows * img.cols;
    ftk_layout L;
    const auto s_gx = L.take<short>(px), s_gy = L.take<short>(px);
    const auto s_key = L.take<unsigned long long>(px), s_tmp = L.take<unsigned long long>(px), s_wmax = L.take<unsigned long long>(px);
    const auto s_list = L.take<unsigned long long>((size_t)plan.capacity);
    const auto s_count = L.take<unsigned>(1);
    const auto s_plane = L.take<uint8_t>(occupied.n > 0 ? px : 0), s_dilated = L.take<uint8_t>(occupied.n > 0 ? px : 0);
    const int rc = ftk_ensure_scratch(ctx, L);
    if (rc != FTK_OK) {
        return rc;
    }
    void *base = ctx->scratch.get();
    ftk::HarrisParams p{};
    p.img = img;
    p.gx = s_gx.in(base);
    p.gy = s_gy.in(base);
    p.response = nullptr;
    p.key = s_key.in(base);
    p.tmp = s_tmp.in(base);
    p.wmax = s_wmax.in(base);
    p.list = s_list.in(base);
    p.count = s_count.in(base);
    p.capacity = (unsigned)plan.capacity;
    p.min_distance = min_distance;
    p.min_response = min_response;
    occupied.plane = occupied.n > 0 ? s_plane.in(base) : nullptr;
    occupied.dilated = occupied.n > 0 ? s_dilated.in(base) : nullptr;
    FTK_HIP(ctx, ftk::harris_masked_launch(p, occupied, ctx->stream));
    *list = p.list;
    *count = p.count;
    return FTK_OK;
}

ftk::TrackTable table_of(int32_t n_slots, int64_t *d_ids, float *d_points, float *d_prev_points, uint8_t *d_status, int32_t *d_age, int32_t *d_n_live,
                         int64_t *d_next_id) {
    ftk::TrackTable t{};
    t.ids = reinterpret_cast<long long *>(d_ids);
    t.points = d_points;
    t.prev_points = d_prev_points;
    t.status = d_status;
    t.age = d_age;
    t.n_live = d_n_live;
    t.next_id = reinterpret_cast<long long *>(d_next_id);
    t.n = n_slots;
    return t;
}

}  // namespace

extern "C" {

int ftk_harris_detect_device(ftk_context *ctx, const ftk_pyramid *image, int32_t level, int32_t max_count, int32_t min_distance, float min_response,
                             const float *d_occupied_uv, const uint8_t *d_occupied_flags, int32_t n_occupied, float *d_uv_out, int32_t *d_count_out) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "harris_detect_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_count_out || max_count < 0 || (max_count > 0 && !d_uv_out) || n_occupied < 0 || (n_occupied > 0 && !d_occupied_uv)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "harris_detect_device: bad arguments (max_count %d, %d occupied points)", max_count, n_occupied);
    }
    if (!aligned8(d_uv_out)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "harris_detect_device: d_uv_out must be 8-byte aligned (%p)", (const void *)d_uv_out);
    }
    ftk::TrackTablePlan plan;
    int rc = plan_call(ctx, "harris_detect_device", image, level, min_distance, 0, n_occupied, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    if (max_count > 0) {
        FTK_HIP(ctx, hipMemsetAsync(d_uv_out, 0, sizeof(float) * 2 * (size_t)max_count, ctx->stream));  // the zeros behind the rows
    }
    if (max_count == 0 || plan.capacity == 0) {
        FTK_HIP(ctx, hipMemsetAsync(d_count_out, 0, sizeof(int32_t), ctx->stream));
        return FTK_OK;
    }
    ftk::HarrisOccupied occupied{};
    occupied.uv = d_occupied_uv;
    occupied.flags = d_occupied_flags;
    occupied.n = n_occupied;
    ftk::HarrisRankParams r{};
    unsigned long long *list = nullptr;
    unsigned *count = nullptr;
    rc = detect_survivors(ctx, plan, image->levels[level], min_distance, min_response, occupied, &list, &count);
    if (rc != FTK_OK) {
        return rc;
    }
    r.list = list;
    r.count = count;
    r.capacity = (unsigned)plan.capacity;
    r.cols = image->levels[level].cols;
    r.uv_out = d_uv_out;
    r.count_out = d_count_out;
    r.max_count = max_count;
    FTK_HIP(ctx, ftk::harris_rank_launch(plan, r, ctx->stream));
    return FTK_OK;
}

int ftk_track_table_retire_device(ftk_context *ctx, int32_t n_slots, int64_t *d_ids, float *d_points, float *d_prev_points, uint8_t *d_status,
                                  int32_t *d_age, int32_t *d_n_live, const float *d_tracked_uv, const uint8_t *d_tracked_status,
                                  const float *d_back_uv, const uint8_t *d_back_status, float fb_threshold, int32_t *d_free, int32_t *d_n_free) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "track_table_retire_device: null context");
    }
    FTK_LOCK(ctx);
    if (n_slots < 1 || n_slots > FTK_TRACK_TABLE_MAX_SLOTS) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "track_table_retire_device: %d slots outside 1 .. %d", n_slots, FTK_TRACK_TABLE_MAX_SLOTS);
    }
    if (!d_ids || !d_points || !d_prev_points || !d_status || !d_age || !d_n_live || !d_tracked_uv || !d_tracked_status || !d_free || !d_n_free) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "track_table_retire_device: null buffer");
    }
    if ((d_back_uv == nullptr) != (d_back_status == nullptr)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "track_table_retire_device: d_back_uv and d_back_status go together");
    }
    if (d_back_uv && !(fb_threshold >= 0.0f)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "track_table_retire_device: the forward-backward threshold %g must be >= 0", (double)fb_threshold);
    }
    if (!aligned8(d_points) || !aligned8(d_prev_points) || !aligned8(d_tracked_uv) || !aligned8(d_back_uv)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "track_table_retire_device: the (u, v) arrays must be 8-byte aligned");
    }
    ftk::TrackTablePlanInput in{};
    in.rows = in.cols = 1;
    in.n_slots = n_slots;
    const ftk::TrackTablePlan plan = ftk::track_table_plan(in);
    ftk::TrackRetireParams p{};
    p.t = table_of(n_slots, d_ids, d_points, d_prev_points, d_status, d_age, d_n_live, nullptr);
    p.tracked_uv = d_tracked_uv;
    p.tracked_status = d_tracked_status;
    p.back_uv = d_back_uv;
    p.back_status = d_back_status;
    p.fb_threshold = fb_threshold;
    p.free_slots = d_free;
    p.n_free = d_n_free;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::track_table_retire_launch(plan, p, ctx->stream));
    return FTK_OK;
}

int ftk_track_table_fill_device(ftk_context *ctx, const ftk_pyramid *image, int32_t level, int32_t min_distance, float min_response, int32_t n_slots,
                                int64_t *d_ids, float *d_points, float *d_prev_points, uint8_t *d_status, int32_t *d_age, int32_t *d_n_live,
                                int64_t *d_next_id, const int32_t *d_free, const int32_t *d_n_free) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "track_table_fill_device: null context");
    }
    FTK_LOCK(ctx);
    if (n_slots < 1 || n_slots > FTK_TRACK_TABLE_MAX_SLOTS) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "track_table_fill_device: %d slots outside 1 .. %d", n_slots, FTK_TRACK_TABLE_MAX_SLOTS);
    }
    if (!d_ids || !d_points || !d_prev_points || !d_status || !d_age || !d_n_live || !d_next_id || !d_free || !d_n_free) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "track_table_fill_device: null buffer");
    }
    if (!aligned8(d_points) || !aligned8(d_prev_points)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "track_table_fill_device: the (u, v) arrays must be 8-byte aligned");
    }
    ftk::TrackTablePlan plan;
    int rc = plan_call(ctx, "track_table_fill_device", image, level, min_distance, n_slots, n_slots, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (plan.capacity == 0) {
        return FTK_OK;  // no valid centre: no corner, the table stays as it is
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    ftk::HarrisOccupied occupied{};
    occupied.uv = d_points;  // the live slots block their neighbourhoods
    occupied.ids = reinterpret_cast<const long long *>(d_ids);
    occupied.n = n_slots;
    unsigned long long *list = nullptr;
    unsigned *count = nullptr;
    rc = detect_survivors(ctx, plan, image->levels[level], min_distance, min_response, occupied, &list, &count);
    if (rc != FTK_OK) {
        return rc;
    }
    ftk::HarrisRankParams r{};
    r.list = list;
    r.count = count;
    r.capacity = (unsigned)plan.capacity;
    r.cols = image->levels[level].cols;
    r.t = table_of(n_slots, d_ids, d_points, d_prev_points, d_status, d_age, d_n_live, d_next_id);
    r.free_slots = d_free;
    r.n_free = d_n_free;
    FTK_HIP(ctx, ftk::harris_rank_launch(plan, r, ctx->stream));
    return FTK_OK;
}

}  // extern "C"
