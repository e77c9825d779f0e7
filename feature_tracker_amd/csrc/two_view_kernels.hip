// two_view_kernels.hip — two-view outlier rejection on gfx950: RANSAC on the fundamental matrix, on a homography, or on
// both with the rule that picks one (5.21), everything on the device.  The two models are instances of ONE kernel family: a model is a
// compile-time trait (epipolar_device.h: its sample size, its rows of the 8 x 9 system, its inlier test), the fundamental-only entry is the
// launcher with one slot.
//
//  * two_view_scan_kernel: ONE workgroup lists the participants (status == FTK_TRACKED) in ascending index order (a block scan of
//    per-thread counts, as the track table's retire kernel, no atomic append), with their normalised coordinates and their number M.  ONE
//    scan serves both models.
//  * two_view_hypothesis_kernel<Model>: one lane = one hypothesis.  The sampler is integer logic; the 8 x 9 constraint matrix lives in LDS,
//    [entry][lane], because complete pivoting indexes rows and columns at run time and a register array indexed so goes to scratch;
//    [entry][lane] makes every access of a wave one conflict-free row of 64 words.  The elimination, the null vector and its scaling are
//    epipolar_device.h's ep_null_vector for both models, the tail its ep_store_hypothesis.
//  * two_view_score_kernel<Model>: epipolar_device.h's ep_score_walk (a workgroup stages a tile of 256 participants in LDS, each of its
//    waves walks the tile for 4 hypotheses, ONE integer atomicAdd per workgroup and hypothesis) on a record of one float4 and a model of
//    nine floats.  Integer sums: no result depends on the order.
//  * two_view_select_kernel<SLOTS>: ONE workgroup takes each slot's winner key (epipolar_device.h's ep_winner_keys), denormalises the
//    winner and rewrites the statuses of the participants that are not its inliers.  With two slots it first applies the rule on the two
//    integer counts, and the statuses follow the CHOSEN model.
// Every float operation below is stated in DESIGN.md 5.20 and 5.21 and restated in tests/epipolar_ref.c and tests/two_view_ref.c; the build
// has no contraction (-ffp-contract=off) and correctly rounded division and square root.
#include "epipolar_device.h"

namespace ftk {
namespace {

__global__ void __launch_bounds__(kEpipolarScanBlock) two_view_scan_kernel(const TwoViewParams p) {
    __shared__ int32_t scan[kEpipolarScanBlock];
    ep_scan_participants(scan, p.status, p.n, p.scan_per_thread, p.m, [&](const int at, const int i) {
        const float2 r = reinterpret_cast<const float2 *>(p.ref_uv)[i];
        const float2 c = reinterpret_cast<const float2 *>(p.cur_uv)[i];
        p.list[at] = i;
        p.points[at] = make_float4((r.x - p.cx) * p.s, (r.y - p.cy) * p.s, (c.x - p.cx) * p.s, (c.y - p.cy) * p.s);
    });
}

template <class Model>
__global__ void __launch_bounds__(kEpipolarHypBlock) two_view_hypothesis_kernel(const TwoViewParams p) {
    __shared__ float lds[kEpipolarHypLdsFloats * kEpipolarHypBlock];
    const int lane = threadIdx.x;
    const int h = blockIdx.x * kEpipolarHypBlock + lane;
    if (h >= p.hypotheses) {
        return;  // (no barrier below)
    }
    constexpr int L = kEpipolarHypBlock;
    float *const a = lds + lane;                                     // a[(r * 9 + c) * 64]
    int *const perm = reinterpret_cast<int *>(lds + 72 * L) + lane;  // perm[c * 64]
    float *const fv = lds + 81 * L + lane;                           // fv[c * 64]
    const uint32_t m = (uint32_t)max(p.m[0], 0);
    // the sampler: kSample distinct positions of the participants' list
    uint32_t idx[Model::kSample];
    bool ok = ep_draw<Model::kSample>(p.seed, (uint32_t)h, m, idx);
    if (ok) {
#pragma unroll
        for (int k = 0; k < Model::kSample; ++k) {
            const float4 q = p.points[idx[k]];
            ok = ok && ep_finite(q.x) && ep_finite(q.y) && ep_finite(q.z) && ep_finite(q.w);
            Model::template fill<L>(a, k, q);
        }
    }
    // Gaussian elimination with complete pivoting, the null vector, unit norm (epipolar_device.h)
    float f[9];
    ok = ep_null_vector<L>(a, perm, fv, ok, f);
    const TwoViewSlot out = p.slot[Model::kSlot];
    ep_store_hypothesis(out.models, out.valid, out.counts, h, ok, f);
}

template <class Model>
__global__ void __launch_bounds__(kEpipolarScoreTile) two_view_score_kernel(const TwoViewParams p) {
    __shared__ float4 tile[kEpipolarScoreTile];
    const TwoViewSlot slot = p.slot[Model::kSlot];
    ep_score_walk<9>(
        min(p.m[0], p.n), Model::kSample, p.hypotheses, slot.models, slot.valid, slot.counts,
        [&](const int at, const int j, const bool live) { tile[at] = live ? p.points[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f); },
        [&](const float (&f)[9], const int at) { return Model::inlier(f, tile[at], p.tn2); });
}

// The select kernel's parts, each stated once for its two instances (the winner keys: epipolar_device.h's ep_winner_keys).

// G = M T, T = [s 0 tx; 0 s ty; 0 0 1]: the first half of either denormalisation.
__device__ __forceinline__ void sel_times_T(const float (&f)[9], const float s, const float tx, const float ty, float (&g)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        g[r * 3 + 0] = f[r * 3 + 0] * s;
        g[r * 3 + 1] = f[r * 3 + 1] * s;
        g[r * 3 + 2] = (f[r * 3 + 0] * tx + f[r * 3 + 1] * ty) + f[r * 3 + 2];
    }
}

// F in pixels = T^T F T: G = F T, then T^T G.
__device__ __forceinline__ void sel_pixel_F(const TwoViewParams &p, const float (&f)[9], float (&out)[9]) {
    const float s = p.s, tx = -(p.cx * p.s), ty = -(p.cy * p.s);
    float g[9];
    sel_times_T(f, s, tx, ty, g);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out[0 + c] = s * g[0 + c];
        out[3 + c] = s * g[3 + c];
        out[6 + c] = (tx * g[0 + c] + ty * g[3 + c]) + g[6 + c];
    }
}

// H in pixels = T^-1 H T, T^-1 = [1/s 0 cx; 0 1/s cy; 0 0 1]: G = H T, then T^-1 G.
__device__ __forceinline__ void sel_pixel_H(const TwoViewParams &p, const float (&h)[9], float (&out)[9]) {
    const float s = p.s, tx = -(p.cx * p.s), ty = -(p.cy * p.s);
    const float is = 1.0f / s;
    float g[9];
    sel_times_T(h, s, tx, ty, g);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out[0 + c] = is * g[0 + c] + p.cx * g[6 + c];
        out[3 + c] = is * g[3 + c] + p.cy * g[6 + c];
        out[6 + c] = g[6 + c];
    }
}

// The participants that are no inliers of the model f become FTK_LARGE_RESIDUAL.
template <class Model>
__device__ __forceinline__ void sel_reject(const TwoViewParams &p, const float (&f)[9], const int m, const int tid) {
    for (int j = tid; j < m; j += kEpipolarScanBlock) {
        if (!Model::inlier(f, p.points[j], p.tn2)) {
            const int32_t i = p.list[j];
            if (i >= 0 && i < p.n) {
                p.status[i] = FTK_LARGE_RESIDUAL;
            }
        }
    }
}

template <int SLOTS>
__global__ void __launch_bounds__(kEpipolarScanBlock) two_view_select_kernel(const TwoViewParams p) {
    __shared__ unsigned long long red[SLOTS][kEpipolarScanBlock];
    const int tid = threadIdx.x;
    unsigned long long key[SLOTS];
    ep_winner_keys<SLOTS>(red, p.select_per_thread, p.hypotheses, key, [&](const int s, const int h) -> int32_t {
        if (SLOTS > 1 && p.run[s] == 0) {  // the slot of a model that did not run: no hypothesis (one slot: the entry has no mode)
            p.slot[s].counts[h] = -1;
            for (int e = 0; e < 9; ++e) {
                p.slot[s].models[(size_t)h * 9 + e] = 0.0f;
            }
            return -1;
        }
        return p.slot[s].counts[h];
    });
    const int m = min(p.m[0], p.n);
    if constexpr (SLOTS == 1) {
        if (!ep_key_has_winner(key[0])) {  // no valid hypothesis (with M < 8: none was formed)
            if (tid == 0) {
                p.best[0] = -1;
                p.n_inliers[0] = m;
            }
            if (tid < 9) {
                p.F[tid] = 0.0f;
            }
            return;
        }
        const int h = ep_key_hypothesis(key[0]);
        float f[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            f[e] = p.slot[0].models[(size_t)h * 9 + e];
        }
        if (tid == 0) {
            p.best[0] = h;
            p.n_inliers[0] = ep_key_count(key[0]);
            float F[9];
            sel_pixel_F(p, f, F);
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                p.F[e] = F[e];
            }
        }
        sel_reject<FundamentalModel>(p, f, m, tid);
    } else {
        const bool has_f = ep_key_has_winner(key[0]), has_h = ep_key_has_winner(key[1]);
        const int32_t n_f = has_f ? ep_key_count(key[0]) : m, n_h = has_h ? ep_key_count(key[1]) : m;
        const int h_f = has_f ? ep_key_hypothesis(key[0]) : -1, h_h = has_h ? ep_key_hypothesis(key[1]) : -1;
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
            f[e] = has_f ? p.slot[0].models[(size_t)h_f * 9 + e] : 0.0f;
            g[e] = has_h ? p.slot[1].models[(size_t)h_h * 9 + e] : 0.0f;
        }
        if (tid == 0) {
            p.model[0] = model;
            p.best[0] = h_f;
            p.best[1] = h_h;
            p.n_inliers[0] = n_f;
            p.n_inliers[1] = n_h;
            float F[9], H[9];
            sel_pixel_F(p, f, F);
            sel_pixel_H(p, g, H);
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                p.F[e] = has_f ? F[e] : 0.0f;
                p.H[e] = has_h ? H[e] : 0.0f;
            }
        }
        if (model == kTwoViewHomography) {
            sel_reject<HomographyModel>(p, g, m, tid);
        } else if (model == kTwoViewFundamental) {
            sel_reject<FundamentalModel>(p, f, m, tid);
        }
    }
}

}  // namespace

hipError_t two_view_launch(const TwoViewPlan &plan, const TwoViewParams &p, hipStream_t stream) {
    TwoViewParams q = p;
    q.scan_per_thread = plan.scan_per_thread;
    q.select_per_thread = plan.select_per_thread;
    q.run[kTwoViewFundamental] = plan.run_fundamental;
    q.run[kTwoViewHomography] = plan.run_homography;
    const dim3 score_grid(plan.score_tiles, plan.score_groups);
    hipLaunchKernelGGL(two_view_scan_kernel, dim3(1), dim3(kEpipolarScanBlock), 0, stream, q);
    if (plan.run_fundamental) {
        hipLaunchKernelGGL(two_view_hypothesis_kernel<FundamentalModel>, dim3(plan.hyp_blocks), dim3(kEpipolarHypBlock), 0, stream, q);
    }
    if (plan.run_homography) {
        hipLaunchKernelGGL(two_view_hypothesis_kernel<HomographyModel>, dim3(plan.hyp_blocks), dim3(kEpipolarHypBlock), 0, stream, q);
    }
    if (plan.run_fundamental) {
        hipLaunchKernelGGL(two_view_score_kernel<FundamentalModel>, score_grid, dim3(kEpipolarScoreTile), 0, stream, q);
    }
    if (plan.run_homography) {
        hipLaunchKernelGGL(two_view_score_kernel<HomographyModel>, score_grid, dim3(kEpipolarScoreTile), 0, stream, q);
    }
    if (plan.slots == 1) {
        hipLaunchKernelGGL(two_view_select_kernel<1>, dim3(1), dim3(kEpipolarScanBlock), 0, stream, q);
    } else {
        hipLaunchKernelGGL(two_view_select_kernel<2>, dim3(1), dim3(kEpipolarScanBlock), 0, stream, q);
    }
    return hipGetLastError();
}

}  // namespace ftk
