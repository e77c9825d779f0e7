// epipolar_device.h — the RANSAC stages that the point-set kernels share.  Each is stated here once:
//
//  * ep_finite: every kernel of two_view_kernels.hip, two_view_pose_kernels.hip, pnp_kernels.hip and landmark_table_kernels.hip.
//  * ep_scan_participants(_if): two_view_scan_kernel, pose_scan_kernel, pnp_scan_kernel.
//  * ep_mix32, ep_draw<S> (the hash and the sampler): two_view_hypothesis_kernel<Model>, pnp_hypothesis_kernel, pnp_p3p_hypothesis_kernel.
//  * ep_null_vector_of<R> (Gaussian elimination with complete pivoting): two_view_hypothesis_kernel<Model> (8 x 9), pnp_hypothesis_kernel
//    (11 x 12).
//  * ep_store_hypothesis<F>: the tail of the three hypothesis kernels.
//  * ep_score_walk<F>: two_view_score_kernel<Model>, pnp_score_kernel.
//  * ep_key and its parts, ep_winner_keys<SLOTS>: two_view_select_kernel<SLOTS>, pnp_select_kernel.
//  * FundamentalModel, HomographyModel with ep_inlier, tv_inlier: the two-view filters' models as compile-time traits.
//
// The pose geometry and the reductions of the kernels that follow a RANSAC are pose_device.h's.  Every float operation is stated in
// DESIGN.md 5.20 and 5.21 and restated in tests/epipolar_ref.c and tests/two_view_ref.c; the build has no contraction
// (-ffp-contract=off) and correctly rounded division and square root.
#pragma once

#include "two_view_plan.h"

namespace ftk {

__device__ __forceinline__ bool ep_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// The participants' scan of ONE workgroup of kEpipolarScanBlock threads (two_view_scan_kernel, pose_scan_kernel): the points with
// status == FTK_TRACKED in ascending index order, by a block scan of per-thread counts (no atomic append).  A thread owns per_thread
// (<= 64) consecutive points, its participants one 64-bit mask; store(at, i) places participant `at` of the list, the point i; m[0]
// receives their number.  scan: kEpipolarScanBlock ints of LDS.
// ep_scan_participants_if: the same with the test of a participant given, takes(i).
template <class Takes, class Store>
__device__ __forceinline__ void ep_scan_participants_if(int32_t *const scan, const int n, const int per_thread, int32_t *const m, Takes takes, Store store) {
    const int tid = threadIdx.x;
    const int begin = min(tid * per_thread, n), end = min(begin + per_thread, n);
    unsigned long long mask = 0ull;
    int32_t mine = 0;
    for (int i = begin; i < end; ++i) {
        if (takes(i)) {
            mask |= 1ull << (i - begin);
            ++mine;
        }
    }
    scan[tid] = mine;
    __syncthreads();
    for (int step = 1; step < kEpipolarScanBlock; step <<= 1) {  // inclusive Hillis-Steele scan
        const int32_t add = tid >= step ? scan[tid - step] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    int32_t at = scan[tid] - mine;
    for (int i = begin; i < end; ++i) {
        if ((mask >> (i - begin)) & 1ull) {
            store(at, i);
            ++at;
        }
    }
    if (tid == kEpipolarScanBlock - 1) {
        m[0] = scan[tid];
    }
}

template <class Store>
__device__ __forceinline__ void ep_scan_participants(int32_t *const scan, const uint8_t *const status, const int n, const int per_thread, int32_t *const m,
                                                     Store store) {
    ep_scan_participants_if(scan, n, per_thread, m, [&](const int i) { return status[i] == FTK_TRACKED; }, store);
}

__device__ __forceinline__ uint32_t ep_fmix32(uint32_t x) {  // murmur3's finaliser
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t ep_mix32(uint32_t seed, uint32_t h, uint32_t k, uint32_t a) {
    return ep_fmix32(ep_fmix32(seed + 0x9E3779B9u * (h + 1u)) ^ (0x85EBCA6Bu * (k * (uint32_t)kEpipolarMaxAttempts + a + 1u)));
}

// The sampler: S distinct positions of a list of m participants, kEpipolarMaxAttempts attempts per draw.  false: m < S or a draw ran out.
template <int S>
__device__ __forceinline__ bool ep_draw(uint32_t seed, uint32_t h, uint32_t m, uint32_t (&idx)[S]) {
    bool ok = m >= (uint32_t)S;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        idx[k] = 0u;
        bool found = false;
        for (uint32_t t = 0; ok && !found && t < (uint32_t)kEpipolarMaxAttempts; ++t) {
            const uint32_t j = (uint32_t)(((uint64_t)ep_mix32(seed, h, (uint32_t)k, t) * (uint64_t)m) >> 32);
            bool dup = false;
#pragma unroll
            for (int q = 0; q < k; ++q) {
                dup = dup || idx[q] == j;
            }
            if (!dup) {
                idx[k] = j;
                found = true;
            }
        }
        ok = ok && found;
    }
    return ok;
}

// The Sampson test without the division, q = normalised (x1, y1, x2, y2), f = normalised F row-major.
__device__ __forceinline__ bool ep_inlier(const float (&f)[9], const float4 q, float tn2) {
    const float x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
    if (!(ep_finite(x1) && ep_finite(y1) && ep_finite(x2) && ep_finite(y2))) {
        return false;
    }
    const float a0 = (f[0] * x1 + f[1] * y1) + f[2];  // F x1
    const float a1 = (f[3] * x1 + f[4] * y1) + f[5];
    const float a2 = (f[6] * x1 + f[7] * y1) + f[8];
    const float b0 = (f[0] * x2 + f[3] * y2) + f[6];  // F^T x2
    const float b1 = (f[1] * x2 + f[4] * y2) + f[7];
    const float num = (x2 * a0 + y2 * a1) + a2;
    const float den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
    const float lhs = num * num, rhs = tn2 * den;
    return den > 0.0f && ep_finite(lhs) && ep_finite(rhs) && lhs <= rhs;
}

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

// The models.  kSample: correspondences of a hypothesis; kSlot: the model's slot of TwoViewParams; fill: the rows that the k-th drawn
// correspondence q contributes to the 8 x 9 system a (LDS, a[(r * 9 + c) * L] of this lane); inlier: the test of a participant.
struct FundamentalModel {
    static constexpr int kSample = kEpipolarSample;
    static constexpr int kSlot = kTwoViewFundamental;
    template <int L>
    static __device__ __forceinline__ void fill(float *const a, const int k, const float4 q) {  // one row: the epipolar constraint
        const float x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
        a[(k * 9 + 0) * L] = x2 * x1;
        a[(k * 9 + 1) * L] = x2 * y1;
        a[(k * 9 + 2) * L] = x2;
        a[(k * 9 + 3) * L] = y2 * x1;
        a[(k * 9 + 4) * L] = y2 * y1;
        a[(k * 9 + 5) * L] = y2;
        a[(k * 9 + 6) * L] = x1;
        a[(k * 9 + 7) * L] = y1;
        a[(k * 9 + 8) * L] = 1.0f;
    }
    static __device__ __forceinline__ bool inlier(const float (&f)[9], const float4 q, float tn2) { return ep_inlier(f, q, tn2); }
};

struct HomographyModel {
    static constexpr int kSample = kTwoViewHomSample;
    static constexpr int kSlot = kTwoViewHomography;
    template <int L>
    static __device__ __forceinline__ void fill(float *const a, const int k, const float4 q) {  // two rows: the DLT system
        const float x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
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
    static __device__ __forceinline__ bool inlier(const float (&g)[9], const float4 q, float tn2) { return tv_inlier(g, q, tn2); }
};

// The unit null vector of the R x (R + 1) matrix a (LDS, a[(r * C + c) * L] of this lane, C = R + 1; destroyed), by Gaussian elimination
// with complete pivoting, back substitution with the free unknown 1 and scaling to unit norm.  perm (C ints) and fv (C floats) are this
// lane's LDS scratch, strided by L as a is.  `ok`: the matrix was filled from finite coordinates.  Returns the validity of f; f is zero
// when invalid.  R = 8: the two-view filters' 8 x 9 system; R = 11: the six-point DLT of a projection (pnp_kernels.hip).
template <int R, int L>
__device__ __forceinline__ bool ep_null_vector_of(float *const a, int *const perm, float *const fv, bool ok, float (&f)[R + 1]) {
    constexpr int C = R + 1;
    for (int c = 0; c < C; ++c) {
        perm[c * L] = c;
    }
    for (int s = 0; ok && s < R; ++s) {
        float best = -1.0f;
        int br = s, bc = s;
        for (int r = s; r < R; ++r) {
            for (int c = s; c < C; ++c) {
                const float v = fabsf(a[(r * C + c) * L]);
                if (v > best) {
                    best = v;
                    br = r;
                    bc = c;
                }
            }
        }
        const float piv = a[(br * C + bc) * L];
        if (!ep_finite(piv) || piv == 0.0f) {
            ok = false;
            break;
        }
        if (br != s) {
            for (int c = s; c < C; ++c) {
                const float t = a[(s * C + c) * L];
                a[(s * C + c) * L] = a[(br * C + c) * L];
                a[(br * C + c) * L] = t;
            }
        }
        if (bc != s) {
            for (int r = 0; r < R; ++r) {
                const float t = a[(r * C + s) * L];
                a[(r * C + s) * L] = a[(r * C + bc) * L];
                a[(r * C + bc) * L] = t;
            }
            const int t = perm[s * L];
            perm[s * L] = perm[bc * L];
            perm[bc * L] = t;
        }
        for (int r = s + 1; r < R; ++r) {
            const float mult = a[(r * C + s) * L] / piv;
            for (int c = s + 1; c < C; ++c) {
                a[(r * C + c) * L] = a[(r * C + c) * L] - mult * a[(s * C + c) * L];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < C; ++i) {
        f[i] = 0.0f;
    }
    if (ok) {
        // the null vector: the free (last) column's unknown is 1, the others by back substitution
        float z[C];
        z[R] = 1.0f;
#pragma unroll
        for (int s = R - 1; s >= 0; --s) {
            float acc = a[(s * C + R) * L];
#pragma unroll
            for (int q = s + 1; q < R; ++q) {
                acc = acc + a[(s * C + q) * L] * z[q];
            }
            z[s] = -acc / a[(s * C + s) * L];
        }
#pragma unroll
        for (int q = 0; q < C; ++q) {
            fv[perm[q * L] * L] = z[q];
        }
        float n2 = fv[0] * fv[0];
#pragma unroll
        for (int i = 1; i < C; ++i) {
            n2 = n2 + fv[i * L] * fv[i * L];
        }
        ok = ep_finite(n2) && n2 > 0.0f;
        if (ok) {
            const float inv = 1.0f / sqrtf(n2);
#pragma unroll
            for (int i = 0; i < C; ++i) {
                f[i] = fv[i * L] * inv;
                ok = ok && ep_finite(f[i]);
            }
        }
    }
    return ok;
}

// The 8 x 9 form of the two filters.
template <int L>
__device__ __forceinline__ bool ep_null_vector(float *const a, int *const perm, float *const fv, bool ok, float (&f)[9]) {
    return ep_null_vector_of<8, L>(a, perm, fv, ok, f);
}

// The tail of a hypothesis kernel: hypothesis h's model of F floats (zero when not ok), its validity flag, and its count, 0 for the
// score kernel to add to or -1 for "no hypothesis".
template <int F>
__device__ __forceinline__ void ep_store_hypothesis(float *const models, uint8_t *const valid, int32_t *const counts, const int h, const bool ok,
                                                    const float (&f)[F]) {
#pragma unroll
    for (int i = 0; i < F; ++i) {
        models[(size_t)h * F + i] = ok ? f[i] : 0.0f;
    }
    valid[h] = ok ? 1 : 0;
    counts[h] = ok ? 0 : -1;
}

// The score walk of ONE workgroup of kEpipolarScoreTile threads on tile blockIdx.x of the m participants and group blockIdx.y of the
// hypotheses.  stage(tid, j, live) puts participant j (zeros when not live: past m) at place tid of the caller's tile in LDS; each wave
// then walks the tile for its kEpipolarScoreGroup / 4 hypotheses, whose model of F floats is wave-uniform; inlier(f, place) is the
// caller's test of the staged participant under the model f.  Inliers are counted by ballot and popcount and reach memory as ONE integer
// atomicAdd per workgroup and hypothesis.  With m < sample no hypothesis was formed and nothing is done.
template <int F, class Stage, class Inlier>
__device__ __forceinline__ void ep_score_walk(const int m, const int sample, const int hypotheses, const float *const models, const uint8_t *const valid,
                                              int32_t *const counts, Stage stage, Inlier inlier) {
    const int base = blockIdx.x * kEpipolarScoreTile;
    if (m < sample || base >= m) {
        return;  // the whole workgroup: the grid covers n
    }
    const int tid = threadIdx.x;
    stage(tid, base + tid, base + tid < m);
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    constexpr int kPerWave = kEpipolarScoreGroup / (kEpipolarScoreTile / 64);
    for (int i = 0; i < kPerWave; ++i) {
        const int h = __builtin_amdgcn_readfirstlane((int)blockIdx.y * kEpipolarScoreGroup + wave * kPerWave + i);
        if (h >= hypotheses) {
            break;
        }
        if (!valid[h]) {
            continue;
        }
        float f[F];
#pragma unroll
        for (int e = 0; e < F; ++e) {
            f[e] = models[(size_t)h * F + e];
        }
        int32_t count = 0;
#pragma unroll
        for (int r = 0; r < kEpipolarScoreTile / 64; ++r) {
            const int j = r * 64 + lane;
            const bool in = base + j < m && inlier(f, j);
            count += (int32_t)__popcll(__ballot(in));
        }
        if (lane == 0 && count > 0) {
            atomicAdd(&counts[h], count);
        }
    }
}

// The winner key of hypothesis h with `count` inliers: (count + 1) << 32 | ~h, so that the maximum is the greatest count and, among equals,
// the lowest h.  count = -1 (no hypothesis) gives a key whose upper half is zero, as the key 0 that nothing was folded into.
__device__ __forceinline__ unsigned long long ep_key(const int32_t count, const int h) {
    return ((unsigned long long)(uint32_t)(count + 1) << 32) | (unsigned long long)(~(uint32_t)h);
}
__device__ __forceinline__ bool ep_key_has_winner(const unsigned long long key) { return (key >> 32) != 0ull; }
__device__ __forceinline__ int ep_key_hypothesis(const unsigned long long key) { return (int)(~(uint32_t)(key & 0xFFFFFFFFull)); }
__device__ __forceinline__ int32_t ep_key_count(const unsigned long long key) { return (int32_t)(key >> 32) - 1; }

// key[s] = the maximum of ep_key(count_of(s, h), h) over the hypotheses, for every slot s, by ONE workgroup of kEpipolarScanBlock threads:
// a thread folds its per_thread consecutive hypotheses, then the workgroup takes the maximum in LDS (red).  Every thread returns with
// every key.
template <int SLOTS, class CountOf>
__device__ __forceinline__ void ep_winner_keys(unsigned long long (&red)[SLOTS][kEpipolarScanBlock], const int per_thread, const int hypotheses,
                                               unsigned long long (&key)[SLOTS], CountOf count_of) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        key[s] = 0ull;
    }
    for (int i = 0; i < per_thread; ++i) {
        const int h = tid * per_thread + i;
        if (h < hypotheses) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                const unsigned long long k = ep_key(count_of(s, h), h);
                key[s] = k > key[s] ? k : key[s];
            }
        }
    }
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        red[s][tid] = key[s];
    }
    __syncthreads();
    for (int step = kEpipolarScanBlock / 2; step > 0; step >>= 1) {
        if (tid < step) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                const unsigned long long other = red[s][tid + step];
                if (other > red[s][tid]) {
                    red[s][tid] = other;
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        key[s] = red[s][0];
    }
}

}  // namespace ftk
