// match_table_plan.h — the launch plan and workspace layout of MatchVideoTracker's landmark table (match_table_kernels.hip,
// DESIGN.md 5.28), as track_table_plan.h is the track table's: a pure function of values (no context, no environment, no HIP call),
// small enough to live in the header.  ftk_match_table.cpp plans, the launchers carry the plan out.
#pragma once

#include "ftk_device.h"
#include "ftk_layout.h"
#include "track_table_plan.h"

namespace ftk {

constexpr int kMatchTableMaxSlots = 4096;  // FTK_MATCH_TABLE_MAX_SLOTS: the matchers' row limit, and four flags per thread of the scan
constexpr int kMatchTableMaxDim = 1024;    // FTK_MATCH_TABLE_MAX_DIM
constexpr int kMatchTableScanPerThread = kMatchTableMaxSlots / kTrackRetireBlock;
constexpr int kMatchTableMoveWaves = 4;    // waves of a workgroup of the row movers: one descriptor row each

static_assert(kMatchTableScanPerThread * kTrackRetireBlock == kMatchTableMaxSlots && kMatchTableScanPerThread == 4,
              "the scan workgroup owns at most four consecutive flags per thread");

struct MatchTablePlanInput {
    int32_t n_slots;    // slots of the table
    int32_t rows_cur;   // K: rows of the current set (the query has none: pass 1)
    int32_t dim;        // D
    int32_t aligned16;  // every descriptor base of the call is 16-byte aligned
};
enum class MatchTableRefusal { None, Slots, Rows, Dim };
struct MatchTablePlan {
    MatchTableRefusal refused;  // not None: nothing else is set
    int32_t slots_per_thread;   // consecutive slots (and query rows) a thread of the ONE scan workgroup owns: 1 .. 4
    int32_t rows_per_thread;    // consecutive current rows it owns: 1 .. 4
    int32_t vec;                // descriptor rows move as float4 (D % 4 == 0 and aligned bases); the same bits either way
    uint32_t query_move_blocks;   // workgroups of kMatchTableMoveWaves waves: one wave per query row
    uint32_t update_move_blocks;  // one wave per current row
    int32_t query_launches, update_launches;  // 2 and 2: the scan workgroup, then the row mover
    ftk_slot16<int32_t> cur_slot;  // the workspace (ftk_layout.h): the current rows' slots [K]
    size_t bytes;
};

inline const char *match_table_refusal_name(MatchTableRefusal r) {
    switch (r) {
        case MatchTableRefusal::None: return "none";
        case MatchTableRefusal::Slots: return "slots";
        case MatchTableRefusal::Rows: return "rows";
        case MatchTableRefusal::Dim: return "dim";
    }
    return "?";
}

inline MatchTablePlan match_table_plan(const MatchTablePlanInput &in) {
    MatchTablePlan p{};
    if (in.n_slots < 1 || in.n_slots > kMatchTableMaxSlots) {
        p.refused = MatchTableRefusal::Slots;
        return p;
    }
    if (in.rows_cur < 1 || in.rows_cur > kMatchTableMaxSlots) {
        p.refused = MatchTableRefusal::Rows;
        return p;
    }
    if (in.dim < 1 || in.dim > kMatchTableMaxDim) {
        p.refused = MatchTableRefusal::Dim;
        return p;
    }
    p.refused = MatchTableRefusal::None;
    p.slots_per_thread = (in.n_slots + kTrackRetireBlock - 1) / kTrackRetireBlock;
    p.rows_per_thread = (in.rows_cur + kTrackRetireBlock - 1) / kTrackRetireBlock;
    p.vec = (in.dim % 4 == 0 && in.aligned16) ? 1 : 0;
    p.query_move_blocks = (uint32_t)((in.n_slots + kMatchTableMoveWaves - 1) / kMatchTableMoveWaves);
    p.update_move_blocks = (uint32_t)((in.rows_cur + kMatchTableMoveWaves - 1) / kMatchTableMoveWaves);
    p.query_launches = 2;
    p.update_launches = 2;
    ftk_layout16 ws;  // cannot wrap: K <= 2^12
    p.cur_slot = ws.take<int32_t>((size_t)in.rows_cur);
    p.bytes = ws.bytes();
    return p;
}

// The landmark table: TrackTable's fields, a descriptor per slot and the frames since a slot was last seen.
struct MatchTable {
    TrackTable t;
    float *descriptors;  // [n][dim]
    int32_t *lost;       // [n]
    int32_t dim;
};
struct MatchTableQueryParams {
    MatchTable m;
    float *q_uv;         // [n][2]
    float *q_desc;       // [n][dim]
    int32_t *q_slot;     // [n]
    int32_t *q_count;    // [1]
};
struct MatchTableUpdateParams {
    MatchTable m;
    const int32_t *q_slot;        // [n] as the query wrote it
    const int32_t *q_count;       // [1]
    const int32_t *match_index;   // [n]
    const uint8_t *match_status;  // [n]
    const float *cur_uv;          // [K][2]
    const float *cur_desc;        // [K][dim]
    const int32_t *cur_count;     // [1] or null: all K rows
    int32_t rows_cur;             // K
    int32_t max_lost;
    int32_t *cur_slot;            // [K]: the caller's array, or the workspace's
};
hipError_t match_table_query_launch(const MatchTablePlan &plan, const MatchTableQueryParams &p, hipStream_t stream);
hipError_t match_table_update_launch(const MatchTablePlan &plan, const MatchTableUpdateParams &p, hipStream_t stream);

}  // namespace ftk
