// track_table_kernels.hip — the device-resident track table of KltVideoTracker on gfx950.
//
//  * track_retire_kernel: after the tracker calls of a frame, ONE workgroup decides which slots stay live, moves their points on and
//    lists the empty slots in ascending slot order (a block scan of per-thread counts, no atomic append), with their number.
//  * harris_rank_kernel: the strongest-K selection of masked detection without a sort and without the host.  The collect pass
//    (feature_kernels.hip) appends the survivors' 64-bit keys in whatever order its atomicAdd hands out; keys are unique (they carry
//    the pixel index), so a survivor's rank is the number of survivors with a greater key, counted all against all over LDS tiles.
//    Rank r writes row r of the detector's output, or (fill) slot free[r] of the table: the result does not depend on the list's order.
//  * track_advance_kernel: one thread, after a fill: next_id and n_live move on by the number of slots filled.
#include "track_table_plan.h"

namespace ftk {
namespace {

__global__ void __launch_bounds__(kTrackRetireBlock) track_retire_kernel(const TrackRetireParams p) {
    __shared__ int32_t scan[kTrackRetireBlock];
    const int tid = threadIdx.x;
    const int n = p.t.n;
    const int begin = min(tid * p.per_thread, n), end = min(begin + p.per_thread, n);
    const float t2 = p.fb_threshold * p.fb_threshold;
    unsigned long long dead_mask = 0ull;
    int32_t dead = 0;
    for (int s = begin; s < end; ++s) {
        bool live = false;
        if (p.t.ids[s] >= 0) {
            const float2 old = reinterpret_cast<const float2 *>(p.t.points)[s];
            const float2 now = reinterpret_cast<const float2 *>(p.tracked_uv)[s];
            uint8_t st = p.tracked_status[s];
            live = st == FTK_TRACKED;
            if (live && p.back_uv) {
                const float2 back = reinterpret_cast<const float2 *>(p.back_uv)[s];
                const float dx = back.x - old.x, dy = back.y - old.y;
                if (!(p.back_status[s] == FTK_TRACKED && fmaf(dy, dy, dx * dx) <= t2)) {
                    live = false;
                    st = FTK_LARGE_RESIDUAL;
                }
            }
            reinterpret_cast<float2 *>(p.t.points)[s] = now;
            p.t.status[s] = st;
            if (live) {
                reinterpret_cast<float2 *>(p.t.prev_points)[s] = old;
                p.t.age[s] += 1;
            } else {
                p.t.ids[s] = -1;
            }
        }
        if (!live) {
            dead_mask |= 1ull << (s - begin);
            ++dead;
        }
    }
    // inclusive scan of the per-thread counts (Hillis-Steele over the workgroup's 1 024 entries)
    scan[tid] = dead;
    __syncthreads();
    for (int step = 1; step < kTrackRetireBlock; step <<= 1) {
        const int32_t add = tid >= step ? scan[tid - step] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    int32_t at = scan[tid] - dead;
    for (int s = begin; s < end; ++s) {
        if ((dead_mask >> (s - begin)) & 1ull) {
            p.free_slots[at++] = s;
        }
    }
    if (tid == kTrackRetireBlock - 1) {
        p.n_free[0] = scan[tid];
        p.t.n_live[0] = n - scan[tid];
    }
}

__global__ void __launch_bounds__(kHarrisRankTile) harris_rank_kernel(const HarrisRankParams p) {
    __shared__ unsigned long long tile[kHarrisRankTile];
    const unsigned survivors = min(p.count[0], p.capacity);
    const unsigned first = blockIdx.x * kHarrisRankTile;
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.count_out) {
        p.count_out[0] = (int32_t)min(survivors, (unsigned)p.max_count);
    }
    if (first >= survivors) {
        return;  // the whole workgroup: the grid covers the list's capacity
    }
    const unsigned i = first + threadIdx.x;
    const unsigned long long mine = i < survivors ? p.list[i] : 0ull;
    unsigned rank = 0;
    for (unsigned base = 0; base < survivors; base += kHarrisRankTile) {
        const unsigned j = base + threadIdx.x;
        tile[threadIdx.x] = j < survivors ? p.list[j] : 0ull;  // 0 is no key: it is greater than nobody
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < kHarrisRankTile; ++k) {
            rank += tile[k] > mine ? 1u : 0u;
        }
        __syncthreads();
    }
    if (i >= survivors) {
        return;
    }
    const unsigned idx = 0xFFFFFFFFu - (unsigned)(mine & 0xFFFFFFFFull);
    const float u = (float)(idx % (unsigned)p.cols), v = (float)(idx / (unsigned)p.cols);
    if (p.uv_out) {
        if (rank < (unsigned)p.max_count) {
            reinterpret_cast<float2 *>(p.uv_out)[rank] = make_float2(u, v);
            if (p.score_out) {  // sortable_bits (feature_kernels.hip) undone
                const unsigned s = (unsigned)(mine >> 32);
                p.score_out[rank] = __uint_as_float((s & 0x80000000u) ? (s ^ 0x80000000u) : ~s);
            }
        }
        return;
    }
    const int32_t n_free = min(max(p.n_free[0], 0), p.t.n);
    if (rank < (unsigned)n_free) {
        const int32_t slot = p.free_slots[rank];
        if (slot >= 0 && slot < p.t.n) {
            p.t.ids[slot] = p.t.next_id[0] + (long long)rank;
            reinterpret_cast<float2 *>(p.t.points)[slot] = make_float2(u, v);
            reinterpret_cast<float2 *>(p.t.prev_points)[slot] = make_float2(u, v);
            p.t.status[slot] = FTK_NOT_TRACKED;
            p.t.age[slot] = 0;
        }
    }
}

__global__ void track_advance_kernel(const HarrisRankParams p) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int32_t survivors = (int32_t)min(p.count[0], p.capacity);
        const int32_t filled = min(min(max(p.n_free[0], 0), p.t.n), survivors);
        p.t.next_id[0] += filled;
        p.t.n_live[0] += filled;
    }
}

}  // namespace

hipError_t track_table_retire_launch(const TrackTablePlan &plan, const TrackRetireParams &p, hipStream_t stream) {
    if (p.t.n <= 0) {
        return hipSuccess;
    }
    TrackRetireParams q = p;
    q.per_thread = plan.retire_per_thread;
    hipLaunchKernelGGL(track_retire_kernel, dim3(1), dim3(kTrackRetireBlock), 0, stream, q);
    return hipGetLastError();
}

hipError_t harris_rank_launch(const TrackTablePlan &plan, const HarrisRankParams &p, hipStream_t stream) {
    return harris_rank_launch(plan.rank_blocks, p, stream);
}

hipError_t harris_rank_launch(uint32_t rank_blocks, const HarrisRankParams &p, hipStream_t stream) {
    // (one workgroup at least: with an empty list it still writes the count)
    hipLaunchKernelGGL(harris_rank_kernel, dim3(rank_blocks > 0 ? rank_blocks : 1), dim3(kHarrisRankTile), 0, stream, p);
    if (!p.uv_out) {
        hipLaunchKernelGGL(track_advance_kernel, dim3(1), dim3(64), 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace ftk
