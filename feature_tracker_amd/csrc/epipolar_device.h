// epipolar_device.h — the device functions of the two-view kernels (two_view_kernels.hip): "finite", the hash, the
// sampler, the null vector of an R x (R + 1) system by Gaussian elimination with complete pivoting (8 x 9 here, 11 x 12 in
// pnp_kernels.hip), the two inlier tests, and the two models as compile-time traits of the hypothesis, score and select kernels.  Every float operation is stated in DESIGN.md 5.20 and 5.21 and
// restated in tests/epipolar_ref.c and tests/two_view_ref.c; the build has no contraction (-ffp-contract=off) and correctly rounded
// division and square root.
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

// ---- what PnpRansac (pnp_kernels.hip) and the landmark table (landmark_table_kernels.hip) share ----

// The inlier rule on the camera coordinates c of a landmark seen at the calibrated (x, y).
__device__ __forceinline__ bool pnp_inlier(const float (&c)[3], const float x, const float y, const float ry, const float tn2) {
    const float ex = c[0] - x * c[2];
    const float ey = (c[1] - y * c[2]) * ry;
    const float lhs = ex * ex + ey * ey, rhs = tn2 * (c[2] * c[2]);
    return c[2] > 0.0f && ep_finite(lhs) && ep_finite(rhs) && lhs <= rhs;
}

// R_rc of a unit quaternion, row-major.
__device__ __forceinline__ void pnp_rotation(const float (&q)[7], float (&R)[9]) {
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0f - 2.0f * (y * y + z * z), R[1] = 2.0f * (x * y - w * z), R[2] = 2.0f * (x * z + w * y);
    R[3] = 2.0f * (x * y + w * z), R[4] = 1.0f - 2.0f * (x * x + z * z), R[5] = 2.0f * (y * z - w * x);
    R[6] = 2.0f * (x * z - w * y), R[7] = 2.0f * (y * z + w * x), R[8] = 1.0f - 2.0f * (x * x + y * y);
}

// c = R_rc^T (X - p_rc)
__device__ __forceinline__ void pnp_camera(const float (&R)[9], const float (&ps)[7], const float X, const float Y, const float Z, float (&c)[3]) {
    const float d0 = X - ps[4], d1 = Y - ps[5], d2 = Z - ps[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        c[j] = (R[j] * d0 + R[3 + j] * d1) + R[6 + j] * d2;
    }
}

// The two-ray depths z1, z2 of z2 b = z1 a + t by the 2 x 2 normal equations of the midpoint (TwoViewPose's cheirality test, DESIGN.md
// 5.29; the landmark table's triangulation); aa, bb, ab: the rays' squared lengths and their product, for the caller's
// parallax test.  true: both depths finite and > 0.
__device__ __forceinline__ bool ep_two_ray_depths(const float (&a)[3], const float (&b)[3], const float (&t)[3], float &z1, float &z2, float &aa,
                                                  float &bb, float &ab) {
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    ab = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    const float at = (a[0] * t[0] + a[1] * t[1]) + a[2] * t[2];
    const float bt = (b[0] * t[0] + b[1] * t[1]) + b[2] * t[2];
    const float det = aa * bb - ab * ab;
    z1 = (ab * bt - bb * at) / det;
    z2 = (aa * bt - ab * at) / det;
    return ep_finite(z1) && ep_finite(z2) && z1 > 0.0f && z2 > 0.0f;
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

}  // namespace ftk
