// match_table_kernels.hip — the device-resident landmark table of MatchVideoTracker on gfx950.
//
//  * match_table_query_scan_kernel: ONE workgroup lists the live slots in ascending slot order (a block scan of per-thread counts, no
//    atomic append): q_slot, -1 behind the count, and the count.
//  * match_table_query_move_kernel: one wave per query row gathers the slot's point and descriptor, +0 behind the count.
//  * match_table_update_scan_kernel: ONE workgroup carries a frame's matches into the table.  The claim words (an integer atomicMin per
//    current row, in LDS) decide the hits, the rows' threads move the live slots on, one packed block scan ranks the empty slots and the
//    unclaimed current rows, and rank r of the one goes to rank r of the other.  Everything but the descriptors is written here.
//  * match_table_update_move_kernel: one wave per current row copies its descriptor into the slot it now belongs to.
// Integer logic and copies: the result is a pure function of the inputs, whatever the schedule.
#include <limits.h>

#include "match_table_plan.h"

namespace ftk {
namespace {

constexpr int kBlock = kTrackRetireBlock;
constexpr int kPer = kMatchTableScanPerThread;

// Inclusive scan of one value per thread over the workgroup (Hillis-Steele, as track_retire_kernel's).
__device__ __forceinline__ int32_t block_scan_inclusive(int32_t *scan, int tid, int32_t mine) {
    scan[tid] = mine;
    __syncthreads();
    for (int step = 1; step < kBlock; step <<= 1) {
        const int32_t add = tid >= step ? scan[tid - step] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    return scan[tid];
}

__device__ __forceinline__ int32_t clamp_count(const int32_t *word, int32_t rows) { return word ? min(max(word[0], 0), rows) : rows; }

__global__ void __launch_bounds__(kBlock) match_table_query_scan_kernel(const MatchTableQueryParams p, const int32_t per_thread) {
    __shared__ int32_t scan[kBlock];
    const int tid = threadIdx.x;
    const int n = p.m.t.n;
    const int begin = min(tid * per_thread, n), end = min(begin + per_thread, n);
    unsigned live_mask = 0u;
    int32_t live = 0;
    for (int s = begin; s < end; ++s) {
        if (p.m.t.ids[s] >= 0) {
            live_mask |= 1u << (s - begin);
            ++live;
        }
    }
    const int32_t inclusive = block_scan_inclusive(scan, tid, live);
    const int32_t nq = scan[kBlock - 1];
    int32_t at = inclusive - live;
    for (int s = begin; s < end; ++s) {
        if ((live_mask >> (s - begin)) & 1u) {
            p.q_slot[at++] = s;
        }
    }
    for (int r = begin; r < end; ++r) {  // the rows behind the count: every row of q_slot is written exactly once
        if (r >= nq) {
            p.q_slot[r] = -1;
        }
    }
    if (tid == 0) {
        p.q_count[0] = nq;
    }
}

// Row `row` of dst <- row `from` of src (from < 0: +0), by one wave.
template <bool kVec>
__device__ __forceinline__ void move_row(float *dst, const float *src, int64_t row, int64_t from, int32_t dim, int lane) {
    if (kVec) {
        float4 *d = reinterpret_cast<float4 *>(dst + row * dim);
        const float4 *s = reinterpret_cast<const float4 *>(src + (from < 0 ? 0 : from) * dim);
        for (int c = lane; c < dim / 4; c += kWave) {
            d[c] = from < 0 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : s[c];
        }
    } else {
        float *d = dst + row * dim;
        const float *s = src + (from < 0 ? 0 : from) * dim;
        for (int c = lane; c < dim; c += kWave) {
            d[c] = from < 0 ? 0.0f : s[c];
        }
    }
}

template <bool kVec>
__global__ void __launch_bounds__(kMatchTableMoveWaves *kWave) match_table_query_move_kernel(const MatchTableQueryParams p) {
    const int lane = threadIdx.x % kWave;
    const int r = blockIdx.x * kMatchTableMoveWaves + threadIdx.x / kWave;
    const int n = p.m.t.n;
    if (r >= n) {
        return;
    }
    int32_t s = p.q_slot[r];
    if (s < 0 || s >= n) {
        s = -1;
    }
    if (lane == 0) {
        reinterpret_cast<float2 *>(p.q_uv)[r] = s < 0 ? make_float2(0.0f, 0.0f) : reinterpret_cast<const float2 *>(p.m.t.points)[s];
    }
    move_row<kVec>(p.q_desc, p.m.descriptors, r, s, p.m.dim, lane);
}

__global__ void __launch_bounds__(kBlock) match_table_update_scan_kernel(const MatchTableUpdateParams p, const int32_t slots_per_thread,
                                                                         const int32_t rows_per_thread) {
    __shared__ int32_t scan[kBlock];
    __shared__ int32_t claim[kMatchTableMaxSlots];     // per current row: the lowest TRACKED row that names it; later the empty slots in order
    __shared__ int32_t slot_of[kMatchTableMaxSlots];   // per current row: the slot it now belongs to, or -1
    __shared__ uint8_t named[kMatchTableMaxSlots];     // per current row: some row names it
    __shared__ uint8_t empty[kMatchTableMaxSlots];     // per slot: empty (before the call, or retired by it)
    const int tid = threadIdx.x;
    const int n = p.m.t.n, K = p.rows_cur;
    const int nq = clamp_count(p.q_count, n), nk = clamp_count(p.cur_count, K);
    const int s_begin = min(tid * slots_per_thread, n), s_end = min(s_begin + slots_per_thread, n);
    const int j_begin = min(tid * rows_per_thread, K), j_end = min(j_begin + rows_per_thread, K);
    for (int s = s_begin; s < s_end; ++s) {
        empty[s] = p.m.t.ids[s] < 0 ? 1 : 0;
    }
    for (int j = j_begin; j < j_end; ++j) {
        claim[j] = INT_MAX;
        slot_of[j] = -1;
        named[j] = 0;
    }
    __syncthreads();
    // 1. claiming: the rows are the slots' index space too (nq <= n), so a thread's rows are its s_begin .. s_end
    int32_t names[kPer];
    for (int k = 0; k < kPer; ++k) {
        const int r = s_begin + k;
        names[k] = -1;
        if (r < s_end && r < nq) {
            const int32_t j = p.match_index[r];
            if (j >= 0 && j < nk) {
                names[k] = j;
                named[j] = 1;  // (several rows may store the same byte)
                if (p.match_status[r] == FTK_TRACKED) {
                    atomicMin(&claim[j], r);
                }
            }
        }
    }
    __syncthreads();
    // 2. the live slots
    for (int k = 0; k < kPer; ++k) {
        const int r = s_begin + k;
        if (!(r < s_end && r < nq)) {
            continue;
        }
        const int32_t s = p.q_slot[r];
        if (s < 0 || s >= n || empty[s]) {  // (a slot that was empty before the call is not touched here)
            continue;
        }
        const int32_t j = names[k];
        if (j >= 0 && claim[j] == r) {
            float2 *points = reinterpret_cast<float2 *>(p.m.t.points);
            reinterpret_cast<float2 *>(p.m.t.prev_points)[s] = points[s];
            points[s] = reinterpret_cast<const float2 *>(p.cur_uv)[j];
            p.m.t.age[s] += 1;
            p.m.lost[s] = 0;
            p.m.t.status[s] = FTK_TRACKED;
            slot_of[j] = s;
        } else {
            const int32_t lost = p.m.lost[s] + 1;
            p.m.lost[s] = lost;
            p.m.t.status[s] = FTK_LARGE_RESIDUAL;
            if (lost > p.max_lost) {
                p.m.t.ids[s] = -1;
                empty[s] = 1;
            }
        }
    }
    __syncthreads();
    // 3. admission: one scan of two packed counts (each at most 4 096: 16 bits hold them), the empty slots below, the unclaimed rows above
    int32_t n_empty = 0, n_unclaimed = 0;
    for (int s = s_begin; s < s_end; ++s) {
        n_empty += empty[s];
    }
    for (int j = j_begin; j < j_end; ++j) {
        n_unclaimed += (j < nk && !named[j]) ? 1 : 0;
    }
    const int32_t inclusive = block_scan_inclusive(scan, tid, n_empty | (n_unclaimed << 16));
    const int32_t total = scan[kBlock - 1];
    const int32_t total_empty = total & 0xFFFF, total_unclaimed = total >> 16;
    const int32_t admitted = min(total_empty, total_unclaimed);
    int32_t *empty_list = claim;  // (the claim words were last read before the barrier above)
    int32_t at = (inclusive & 0xFFFF) - n_empty;
    for (int s = s_begin; s < s_end; ++s) {
        if (empty[s]) {
            empty_list[at++] = s;
        }
    }
    __syncthreads();
    const long long next_id = p.m.t.next_id[0];
    int32_t rank = (inclusive >> 16) - n_unclaimed;
    for (int j = j_begin; j < j_end; ++j) {
        if (j < nk && !named[j]) {
            if (rank < admitted) {
                const int32_t s = empty_list[rank];
                const float2 uv = reinterpret_cast<const float2 *>(p.cur_uv)[j];
                p.m.t.ids[s] = next_id + rank;
                reinterpret_cast<float2 *>(p.m.t.points)[s] = uv;
                reinterpret_cast<float2 *>(p.m.t.prev_points)[s] = uv;
                p.m.t.age[s] = 0;
                p.m.lost[s] = 0;
                p.m.t.status[s] = FTK_NOT_TRACKED;
                slot_of[j] = s;
            }
            ++rank;
        }
    }
    __syncthreads();  // (next_id is read by every thread before thread 0 moves it on; slot_of is complete)
    for (int j = j_begin; j < j_end; ++j) {
        p.cur_slot[j] = slot_of[j];
    }
    if (tid == 0) {
        p.m.t.next_id[0] = next_id + admitted;
        p.m.t.n_live[0] = n - total_empty + admitted;
    }
}

template <bool kVec>
__global__ void __launch_bounds__(kMatchTableMoveWaves *kWave) match_table_update_move_kernel(const MatchTableUpdateParams p) {
    const int lane = threadIdx.x % kWave;
    const int j = blockIdx.x * kMatchTableMoveWaves + threadIdx.x / kWave;
    if (j >= p.rows_cur) {
        return;
    }
    const int32_t s = p.cur_slot[j];
    if (s < 0 || s >= p.m.t.n) {
        return;
    }
    move_row<kVec>(p.m.descriptors, p.cur_desc, s, j, p.m.dim, lane);
}

}  // namespace

hipError_t match_table_query_launch(const MatchTablePlan &plan, const MatchTableQueryParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(match_table_query_scan_kernel, dim3(1), dim3(kBlock), 0, stream, p, plan.slots_per_thread);
    const dim3 grid(plan.query_move_blocks), block(kMatchTableMoveWaves * kWave);
    if (plan.vec) {
        hipLaunchKernelGGL(match_table_query_move_kernel<true>, grid, block, 0, stream, p);
    } else {
        hipLaunchKernelGGL(match_table_query_move_kernel<false>, grid, block, 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t match_table_update_launch(const MatchTablePlan &plan, const MatchTableUpdateParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(match_table_update_scan_kernel, dim3(1), dim3(kBlock), 0, stream, p, plan.slots_per_thread, plan.rows_per_thread);
    const dim3 grid(plan.update_move_blocks), block(kMatchTableMoveWaves * kWave);
    if (plan.vec) {
        hipLaunchKernelGGL(match_table_update_move_kernel<true>, grid, block, 0, stream, p);
    } else {
        hipLaunchKernelGGL(match_table_update_move_kernel<false>, grid, block, 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace ftk
