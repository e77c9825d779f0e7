// raft_warm_kernels.hip — the warm start of RAFT on video: a coarse flow pushed forward along itself, what upstream
// RAFT's forward_interpolate does on the host with scipy.interpolate.griddata(method="nearest").  Every source pixel lands at
// (x + flow.x, y + flow.y); every target pixel takes both flow components of the valid landing nearest to it, the lowest source index
// among equal distances; a batch entry without a valid landing is all +0.
//
// flow_warm_scan_kernel: a workgroup of 256 threads owns kTile = 256 consecutive targets of one batch entry, a lane per target, and one
// of `splits` contiguous ranges of the sources.  The range is staged through LDS kTile landings at a time, one per thread, as (x1, y1);
// an invalid source is staged as (NaN, NaN), whose distance is NaN and never passes the strict `<`.  The scan reads one LDS address per
// step in every lane (a broadcast) and keeps a running (d2, s) under strict `<` in ascending s.  With one split the lane then copies
// the winner's two floats to the output; with more it stores its key (bits(d2) << 32 | s: the bits of a non-negative float order like
// the float, the low word breaks ties towards the lowest index) to its split's slab of the workspace, and flow_warm_gather_kernel takes
// the least key of a target's slabs.  No atomics: every word of the workspace that the gather reads was stored by the scan of the same
// call, so there is nothing to initialise and nothing stale.
// Control flow: every thread of a workgroup reaches every __syncthreads (the trip counts depend on blockIdx alone); a target past H W only
// stops storing.  Addresses: a source index is below H W <= 2^20 by construction of the ranges, the winner's index is one of them.
// Arithmetic: the contract's sequence of correctly rounded float32 operations (-ffp-contract=off), bit-identical to the scalar
// restatement (tests/flow_warm_ref.c).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ftk_device.h"

namespace ftk {
namespace {

constexpr int kTile = kFlowWarmTile;
static_assert(kTile == FTK_FLOW_WARM_TILE, "include/ftk.h states the tile");
static_assert(kTile % 64 == 0, "whole waves");
constexpr uint32_t kNone = 0xffffffffu;  // the low word of a key that no valid source has replaced

__device__ __forceinline__ unsigned long long key_of(float d2, uint32_t s) {
    return ((unsigned long long)__float_as_uint(d2) << 32) | s;
}

// The two output floats of target t: copies of source s's, or +0 without one.
__device__ __forceinline__ void store_winner(const FlowWarmParams &prm, int64_t b, int64_t HW, int t, uint32_t s) {
    const float *in = prm.flow + b * 2 * HW;
    float *out = prm.out + b * 2 * HW;
    const bool any = s != kNone;
    out[t] = any ? in[s] : 0.0f;
    out[HW + t] = any ? in[HW + s] : 0.0f;
}

template <bool kDirect>
__global__ __launch_bounds__(kTile) void flow_warm_scan_kernel(FlowWarmParams prm, int tiles) {
    __shared__ float2 landing[kTile];
    const int tid = threadIdx.x;
    const int W = prm.W, HW = prm.H * prm.W;
    const int split = blockIdx.x % prm.splits;
    const int tile = (blockIdx.x / prm.splits) % tiles;
    const int64_t b = blockIdx.x / prm.splits / tiles;
    const float *fx = prm.flow + b * 2 * HW, *fy = fx + HW;
    const float w = (float)W, h = (float)prm.H;

    const int t = tile * kTile + tid;
    const float tx = (float)(t % W), ty = (float)(t / W);
    float best = __uint_as_float(0x7f800000u);  // +inf: every valid source is nearer
    uint32_t best_s = kNone;

    const int begin = split * prm.split_sources, end = min(begin + prm.split_sources, HW);
    for (int base = begin; base < end; base += kTile) {
        const int s = base + tid;
        float2 l = make_float2(__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u));
        if (s < end) {
            const float x1 = (float)(s % W) + fx[s], y1 = (float)(s / W) + fy[s];
            if (x1 > 0.0f && x1 < w && y1 > 0.0f && y1 < h) {
                l = make_float2(x1, y1);
            }
        }
        __syncthreads();  // the previous tile has been read
        landing[tid] = l;
        __syncthreads();
        const int count = min(kTile, end - base);
#pragma unroll 8
        for (int k = 0; k < count; ++k) {
            const float2 p = landing[k];
            const float ex = tx - p.x, ey = ty - p.y;
            const float d2 = fmaf(ey, ey, ex * ex);
            if (d2 < best) {
                best = d2;
                best_s = (uint32_t)(base + k);
            }
        }
    }
    if (t < HW) {
        if (kDirect) {
            store_winner(prm, b, HW, t, best_s);
        } else {
            prm.workspace[((int64_t)split * prm.B + b) * HW + t] = key_of(best, best_s);
        }
    }
}

__global__ __launch_bounds__(kTile) void flow_warm_gather_kernel(FlowWarmParams prm, int tiles) {
    const int HW = prm.H * prm.W;
    const int64_t b = blockIdx.x / tiles;
    const int t = (blockIdx.x % tiles) * kTile + threadIdx.x;
    if (t >= HW) {
        return;
    }
    unsigned long long key = prm.workspace[b * HW + t];
    for (int k = 1; k < prm.splits; ++k) {
        const unsigned long long other = prm.workspace[((int64_t)k * prm.B + b) * HW + t];
        key = other < key ? other : key;
    }
    store_winner(prm, b, HW, t, (uint32_t)key);
}

}  // namespace

int flow_warm_auto_splits(int32_t B, int32_t H, int32_t W) {
    const int64_t HW = (int64_t)H * W;
    const int64_t tiles = (HW + kTile - 1) / kTile;
    const int64_t wanted = (kFlowWarmFillGroups + tiles * B - 1) / (tiles * B);  // workgroups of targets alone: tiles * B
    const int64_t splits = wanted < tiles ? wanted : tiles;                      // a split scans at least one LDS tile of sources
    return (int)(splits < kFlowWarmMaxSplits ? splits : kFlowWarmMaxSplits);
}

hipError_t flow_warm_launch(const FlowWarmParams &params, hipStream_t stream) {
    FlowWarmParams p = params;
    const int64_t HW = (int64_t)p.H * p.W;
    const int64_t tiles = (HW + kTile - 1) / kTile;
    const int64_t groups = tiles * p.B * p.splits;
    if (p.splits < 1 || HW > kFlowWarmMaxPixels || groups < 1 || groups > 0x7fffffff) {
        return hipErrorInvalidValue;
    }
    // whole LDS tiles of sources per split; a forced split count above the tiles leaves the last ranges empty, which is harmless
    p.split_sources = (int32_t)(((HW + p.splits - 1) / p.splits + kTile - 1) / kTile * kTile);
    if (p.splits == 1) {
        hipLaunchKernelGGL(flow_warm_scan_kernel<true>, dim3((unsigned)groups), dim3(kTile), 0, stream, p, (int)tiles);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(flow_warm_scan_kernel<false>, dim3((unsigned)groups), dim3(kTile), 0, stream, p, (int)tiles);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        return e;
    }
    hipLaunchKernelGGL(flow_warm_gather_kernel, dim3((unsigned)(tiles * p.B)), dim3(kTile), 0, stream, p, (int)tiles);
    return hipGetLastError();
}

}  // namespace ftk
