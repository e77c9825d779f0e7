// klt_scalar.h — the reference's scalar semantics on the device (x86 float->int, wrapping adds, the 24-bit products, the
// fast variants' step bookkeeping) and the handle of a feature's workgroup (Blk, its barrier, lane broadcast, wave priority).
// Used by the three tracker translation units (klt_kernels.hip, klt_basic_kernels.hip, klt_fast_kernels.hip) and, through
// klt_ldlt.h, by direct_kernels.hip.
#pragma once

#include "ftk_device.h"

#include <limits.h>
#include <stddef.h>

namespace ftk {
namespace {

// static_cast<int32_t>(float) as x86-64 cvttss2si does it (out of range / NaN -> INT_MIN)
__device__ __forceinline__ int f2i(float x) { return (x >= -2147483648.0f && x < 2147483648.0f) ? (int)x : INT_MIN; }
__device__ __forceinline__ int wadd(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
// Product of two SMALL integers (patch / window geometry, pixel and row indices inside them: |x| < 2^23, product < 2^31): the
// 24-bit multiplier issues at full rate, v_mul_lo_u32 at a quarter of it — and the kernels are bound by vector issue.
__device__ __forceinline__ int imul(int a, int b) { return __mul24(a, b); }
// __ballot() takes an int: a bool predicate goes through v_cndmask 0/1 + v_cmp_ne before it becomes the lane mask it already was.
__device__ __forceinline__ unsigned long long wave_ballot(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }
__device__ __forceinline__ float floor_from_trunc(float x, int t) {
    const float f = (float)t;
    return (f > x) ? f - 1.0f : f;
}
// 32-bit offset on the 24-bit multiplier (levels are < 2^24 on a side and < 2^32 pixels: checked where a pyramid is made), so the
// load is base + zero-extended offset instead of a quarter-rate 64-bit multiply-add per tap
__device__ __forceinline__ float px(const DevImage &im, int row, int col) { return (float)im.data[__umul24((unsigned)row, (unsigned)im.cols) + (unsigned)col]; }
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Thread coordinates inside the feature's workgroup.
struct Blk {
    int tid, nt, lane, wave, nwaves;
    bool solo = false;  // compile-time true in the one-wave instantiations: no workgroup barrier anywhere, cross-wave exchanges fold away
    bool tree = false;  // throughput mode (KltParams::tree): sums by per-lane partials + a butterfly instead of the exact-order chain
};

// Workgroup barrier; for a one-wave feature only a compiler fence (LDS operations of one wave execute in program order).
__device__ __forceinline__ void blk_sync(const Blk &b) {
    if (b.solo) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

// Returns x behind an optimisation barrier: per-thread index math derived from it is recomputed where
// it is used instead of being hoisted out of the level loop and held in VGPRs for the whole kernel.
__device__ __forceinline__ int opaque(int x) {
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ Blk opaque_blk(const Blk &b) {
    Blk o = b;
    o.tid = opaque(b.tid);
    o.lane = opaque(b.lane);
    return o;
}

// The argument block is ~0.7 KB = a dozen 64-byte lines of the scalar cache, cold at the start of a launch, and the compiler loads a
// field where it is first needed — a dependent miss (an L2 round trip) every few dozen instructions of the prologue, for every
// wave of the launch at once.  One dword of every line is requested up front instead: the misses overlap into one round trip and
// the later loads hit.
template <size_t kBytes>
__device__ __forceinline__ void klt_touch_kernarg() {
    const __attribute__((address_space(4))) uint32_t *ka = (const __attribute__((address_space(4))) uint32_t *)__builtin_amdgcn_kernarg_segment_ptr();
    uint32_t sink = 0;
#pragma unroll
    for (size_t off = 0; off < kBytes; off += 64) {
        sink |= ka[off / 4];
    }
    asm volatile("" ::"s"(sink));
}

// All features of a call are resident at once and the hardware arbitrates oldest-wave-first, which
// lets the first-dispatched features finish early and leaves the youngest ones to run the tail
// alone at single-wave issue rate.  Waves therefore raise their own priority while they are
// behind (coarse pyramid level) and lower it as they advance: the co-resident features progress
// evenly and the last one finishes ~10 % earlier (measured: 53.9 -> 49.3 us span at 2000 features).
// `younger`: the workgroup sits in the later-dispatched half of the launch.  With 2 000 identical features the finishing time
// still correlates 0.87 with the launch slot (31 us for the first 250 workgroups, 36 for the last 250, all started within
// 0.4 us: per-workgroup timestamps), so the younger half runs one step above the older half of the same level:
// config 2 40.4 -> 39.0 us per step, 300 / 1 000-feature launches -3.5 %, config 5 shard -1.7 %, config 1 +-0.  (Rotating or
// purely age-based priorities, and a finer split, all lose: docs/LAB_NOTES.md.)
__device__ __forceinline__ void set_level_priority(int level, bool younger = false) {
    const int pr = (level >= 3 ? 3 : level) + (younger ? 1 : 0);
    if (pr >= 3) {
        __builtin_amdgcn_s_setprio(3);
    } else if (pr == 2) {
        __builtin_amdgcn_s_setprio(2);
    } else if (pr == 1) {
        __builtin_amdgcn_s_setprio(1);
    } else {
        __builtin_amdgcn_s_setprio(0);
    }
}

template <typename T>
__device__ __forceinline__ void swap_values(T &a, T &b) {
    const T t = a;
    a = b;
    b = t;
}

// The value lane `src_lane` holds, wave-uniform (v_readlane: the result lives in an SGPR).
__device__ __forceinline__ float bcast_lane(float v, int src_lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane)); }

// Large-step / convergence bookkeeping shared by the three fast variants
// (basic_klt_fast.cpp:49-60, affine_klt_fast.cpp:55-67, lssd_klt_fast.cpp:101-112).
// Returns true when the iteration loop has to stop.
__device__ __forceinline__ bool fast_step_logic(const KltParams &p, float squared_step, float &last_squared_step, uint32_t &large_step_cnt,
                                                uint8_t &status) {
    if (squared_step < last_squared_step) {
        last_squared_step = squared_step;
        large_step_cnt = 0;
    } else {
        ++large_step_cnt;
        if (large_step_cnt >= p.max_large_step) {
            return true;
        }
    }
    if (squared_step < p.converge) {
        status = FTK_TRACKED;
        return true;
    }
    return false;
}

}  // namespace
}  // namespace ftk
