// two_view_kernels.hip — two-view outlier rejection with a choice of model on gfx950: the homography next to the
// fundamental matrix of epipolar_kernels.hip, fitted by the same RANSAC on the same participants and seed, and the rule that picks one.
//
//  * The scan, and the fundamental route's hypothesis and score kernels, are epipolar_kernels.hip's own (epipolar_launch_*): ONE scan
//    serves both models.
//  * two_view_homography_hypothesis_kernel: one lane = one hypothesis.  Four draws of the shared sampler fill the 8 x 9 DLT system in LDS,
//    [entry][lane]; the elimination, the null vector and its scaling are epipolar_device.h's ep_null_vector, the function the fundamental
//    route calls.
//  * two_view_homography_score_kernel: epipolar_score_kernel's shape (a tile of 256 participants in LDS, 4 wave-uniform models per wave,
//    ballot + popcount, ONE integer atomicAdd per workgroup and hypothesis) with the one-sided transfer error.
//  * two_view_select_kernel: ONE workgroup takes the maximum of (count + 1) << 32 | ~h of each model that ran, applies the rule on the two
//    integer counts, denormalises both winners and rewrites the statuses of the participants that are not inliers of the CHOSEN model.
// Every float operation below is stated in DESIGN.md 5.21 and restated in tests/two_view_ref.c; the build has no contraction.
#include "epipolar_device.h"
#include "two_view_plan.h"

namespace ftk {
namespace {

// The one-sided transfer error in the current image without the division, q = normalised (x1, y1, x2, y2), g = normalised H row-major.
__device__ __forceinline__ bool tv_inlier(const float (&g)[9], const float4 q, float tn2) {
    const float x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
    if (!(ep_finite(x1) && ep_finite(y1) && ep_finite(x2) && ep_finite(y2))) {
        return false;
    }
    const float w = (g[6] * x1 + g[7] * y1) + g[8];
    const float px = (g[0] * x1 + g[1] * y1) + g[2];
    const float py = (g[3] * x1 + g[4] * y1) + g[5];
    const float ex = px - x2 * w;
    const float ey = py - y2 * w;
    const float lhs = ex * ex + ey * ey, rhs = tn2 * (w * w);
    return w != 0.0f && ep_finite(lhs) && ep_finite(rhs) && lhs <= rhs;
}

__global__ void __launch_bounds__(kEpipolarHypBlock) two_view_homography_hypothesis_kernel(const TwoViewParams p) {
    __shared__ float lds[kEpipolarHypLdsFloats * kEpipolarHypBlock];
    const int lane = threadIdx.x;
    const int h = blockIdx.x * kEpipolarHypBlock + lane;
    if (h >= p.e.hypotheses) {
        return;  // (no barrier below)
    }
    constexpr int L = kEpipolarHypBlock;
    float *const a = lds + lane;                                     // a[(r * 9 + c) * 64]
    int *const perm = reinterpret_cast<int *>(lds + 72 * L) + lane;  // perm[c * 64]
    float *const fv = lds + 81 * L + lane;                           // fv[c * 64]
    const uint32_t m = (uint32_t)max(p.e.m[0], 0);
    uint32_t idx[kTwoViewHomSample];
    bool ok = ep_draw<kTwoViewHomSample>(p.e.seed, (uint32_t)h, m, idx);
    if (ok) {
#pragma unroll
        for (int k = 0; k < kTwoViewHomSample; ++k) {
            const float4 q = p.e.points[idx[k]];
            const float x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
            ok = ok && ep_finite(x1) && ep_finite(y1) && ep_finite(x2) && ep_finite(y2);
            const int r0 = 2 * k * 9, r1 = (2 * k + 1) * 9;
            a[(r0 + 0) * L] = x1;
            a[(r0 + 1) * L] = y1;
            a[(r0 + 2) * L] = 1.0f;
            a[(r0 + 3) * L] = 0.0f;
            a[(r0 + 4) * L] = 0.0f;
            a[(r0 + 5) * L] = 0.0f;
            a[(r0 + 6) * L] = -(x2 * x1);
            a[(r0 + 7) * L] = -(x2 * y1);
            a[(r0 + 8) * L] = -x2;
            a[(r1 + 0) * L] = 0.0f;
            a[(r1 + 1) * L] = 0.0f;
            a[(r1 + 2) * L] = 0.0f;
            a[(r1 + 3) * L] = x1;
            a[(r1 + 4) * L] = y1;
            a[(r1 + 5) * L] = 1.0f;
            a[(r1 + 6) * L] = -(y2 * x1);
            a[(r1 + 7) * L] = -(y2 * y1);
            a[(r1 + 8) * L] = -y2;
        }
    }
    float g[9];
    ok = ep_null_vector<L>(a, perm, fv, ok, g);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        p.models_h[(size_t)h * 9 + i] = ok ? g[i] : 0.0f;
    }
    p.valid_h[h] = ok ? 1 : 0;
    p.counts_h[h] = ok ? 0 : -1;
}

__global__ void __launch_bounds__(kEpipolarScoreTile) two_view_homography_score_kernel(const TwoViewParams p) {
    __shared__ float4 tile[kEpipolarScoreTile];
    const int m = min(p.e.m[0], p.e.n);
    const int base = blockIdx.x * kEpipolarScoreTile;
    if (m < kTwoViewHomSample || base >= m) {
        return;  // the whole workgroup: the grid covers n
    }
    const int tid = threadIdx.x;
    tile[tid] = base + tid < m ? p.e.points[base + tid] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    constexpr int kPerWave = kEpipolarScoreGroup / (kEpipolarScoreTile / 64);
    for (int i = 0; i < kPerWave; ++i) {
        const int h = __builtin_amdgcn_readfirstlane((int)blockIdx.y * kEpipolarScoreGroup + wave * kPerWave + i);
        if (h >= p.e.hypotheses) {
            break;
        }
        if (!p.valid_h[h]) {
            continue;
        }
        float g[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            g[e] = p.models_h[(size_t)h * 9 + e];
        }
        int32_t count = 0;
#pragma unroll
        for (int r = 0; r < kEpipolarScoreTile / 64; ++r) {
            const int j = r * 64 + lane;
            const bool in = base + j < m && tv_inlier(g, tile[j], p.e.tn2);
            count += (int32_t)__popcll(__ballot(in));
        }
        if (lane == 0 && count > 0) {
            atomicAdd(&p.counts_h[h], count);
        }
    }
}

__global__ void __launch_bounds__(kEpipolarScanBlock) two_view_select_kernel(const TwoViewParams p) {
    __shared__ unsigned long long red[2][kEpipolarScanBlock];
    const int tid = threadIdx.x;
    const int K = p.e.hypotheses;
    unsigned long long key_f = 0ull, key_h = 0ull;
    for (int i = 0; i < p.e.select_per_thread; ++i) {
        const int h = tid * p.e.select_per_thread + i;
        if (h < K) {
            const unsigned long long low = (unsigned long long)(~(uint32_t)h);
            if (p.run_fundamental) {
                const unsigned long long k = ((unsigned long long)(uint32_t)(p.e.counts[h] + 1) << 32) | low;
                key_f = k > key_f ? k : key_f;
            } else {  // the slot of a model that did not run: no hypothesis
                p.e.counts[h] = -1;
                for (int e = 0; e < 9; ++e) {
                    p.e.models[(size_t)h * 9 + e] = 0.0f;
                }
            }
            if (p.run_homography) {
                const unsigned long long k = ((unsigned long long)(uint32_t)(p.counts_h[h] + 1) << 32) | low;
                key_h = k > key_h ? k : key_h;
            } else {
                p.counts_h[h] = -1;
                for (int e = 0; e < 9; ++e) {
                    p.models_h[(size_t)h * 9 + e] = 0.0f;
                }
            }
        }
    }
    red[0][tid] = key_f;
    red[1][tid] = key_h;
    __syncthreads();
    for (int step = kEpipolarScanBlock / 2; step > 0; step >>= 1) {
        if (tid < step) {
            const unsigned long long of = red[0][tid + step], oh = red[1][tid + step];
            if (of > red[0][tid]) {
                red[0][tid] = of;
            }
            if (oh > red[1][tid]) {
                red[1][tid] = oh;
            }
        }
        __syncthreads();
    }
    key_f = red[0][0];
    key_h = red[1][0];
    const int m = min(p.e.m[0], p.e.n);
    const bool has_f = (key_f >> 32) != 0ull, has_h = (key_h >> 32) != 0ull;
    const int32_t n_f = has_f ? (int32_t)(key_f >> 32) - 1 : m, n_h = has_h ? (int32_t)(key_h >> 32) - 1 : m;
    const int h_f = has_f ? (int)(~(uint32_t)(key_f & 0xFFFFFFFFull)) : -1, h_h = has_h ? (int)(~(uint32_t)(key_h & 0xFFFFFFFFull)) : -1;
    // the rule, on integers: the homography iff it has a winner and (the fundamental matrix has none or 1000 n_H >= p n_F)
    int model = -1;
    if (has_h && (!has_f || 1000ll * (long long)n_h >= (long long)p.prefer_permille * (long long)n_f)) {
        model = kTwoViewHomography;
    } else if (has_f) {
        model = kTwoViewFundamental;
    }
    float f[9], g[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        f[e] = has_f ? p.e.models[(size_t)h_f * 9 + e] : 0.0f;
        g[e] = has_h ? p.models_h[(size_t)h_h * 9 + e] : 0.0f;
    }
    if (tid == 0) {
        p.model[0] = model;
        p.best[0] = h_f;
        p.best[1] = h_h;
        p.n_inliers[0] = n_f;
        p.n_inliers[1] = n_h;
        const float s = p.e.s, tx = -(p.e.cx * p.e.s), ty = -(p.e.cy * p.e.s);
        // F in pixels = T^T F T, T = [s 0 tx; 0 s ty; 0 0 1]: G = F T, then T^T G (5.20)
        float t[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            t[r * 3 + 0] = f[r * 3 + 0] * s;
            t[r * 3 + 1] = f[r * 3 + 1] * s;
            t[r * 3 + 2] = (f[r * 3 + 0] * tx + f[r * 3 + 1] * ty) + f[r * 3 + 2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p.F[0 + c] = has_f ? s * t[0 + c] : 0.0f;
            p.F[3 + c] = has_f ? s * t[3 + c] : 0.0f;
            p.F[6 + c] = has_f ? (tx * t[0 + c] + ty * t[3 + c]) + t[6 + c] : 0.0f;
        }
        // H in pixels = T^-1 H T, T^-1 = [1/s 0 cx; 0 1/s cy; 0 0 1]: G = H T, then T^-1 G
        const float is = 1.0f / s;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            t[r * 3 + 0] = g[r * 3 + 0] * s;
            t[r * 3 + 1] = g[r * 3 + 1] * s;
            t[r * 3 + 2] = (g[r * 3 + 0] * tx + g[r * 3 + 1] * ty) + g[r * 3 + 2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p.H[0 + c] = has_h ? is * t[0 + c] + p.e.cx * t[6 + c] : 0.0f;
            p.H[3 + c] = has_h ? is * t[3 + c] + p.e.cy * t[6 + c] : 0.0f;
            p.H[6 + c] = has_h ? t[6 + c] : 0.0f;
        }
    }
    if (model < 0) {
        return;
    }
    for (int j = tid; j < m; j += kEpipolarScanBlock) {
        const float4 q = p.e.points[j];
        const bool in = model == kTwoViewHomography ? tv_inlier(g, q, p.e.tn2) : ep_inlier(f, q, p.e.tn2);
        if (!in) {
            const int32_t i = p.e.list[j];
            if (i >= 0 && i < p.e.n) {
                p.e.status[i] = FTK_LARGE_RESIDUAL;
            }
        }
    }
}

}  // namespace

hipError_t two_view_launch(const TwoViewPlan &plan, const TwoViewParams &p, hipStream_t stream) {
    TwoViewParams q = p;
    q.e.scan_per_thread = plan.scan_per_thread;
    q.e.select_per_thread = plan.select_per_thread;
    q.run_fundamental = plan.run_fundamental;
    q.run_homography = plan.run_homography;
    epipolar_launch_scan(q.e, stream);
    if (plan.run_fundamental) {
        epipolar_launch_hypotheses(plan.hyp_blocks, q.e, stream);
    }
    if (plan.run_homography) {
        hipLaunchKernelGGL(two_view_homography_hypothesis_kernel, dim3(plan.hyp_blocks), dim3(kEpipolarHypBlock), 0, stream, q);
    }
    if (plan.run_fundamental) {
        epipolar_launch_score(plan.score_tiles, plan.score_groups, q.e, stream);
    }
    if (plan.run_homography) {
        hipLaunchKernelGGL(two_view_homography_score_kernel, dim3(plan.score_tiles, plan.score_groups), dim3(kEpipolarScoreTile), 0, stream, q);
    }
    hipLaunchKernelGGL(two_view_select_kernel, dim3(1), dim3(kEpipolarScanBlock), 0, stream, q);
    return hipGetLastError();
}

}  // namespace ftk
