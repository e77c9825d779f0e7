// dense_flow_kernels.hip — Farneback dense optical flow (feature_tracker::DenseOpticalFlow,
// src/dense_optical_flow_tracker/dense_optical_flow.cpp) on gfx950.
//
// Three launches per pyramid level:
//   dense_moments_kernel  the six Gaussian-weighted moment images of ref AND cur (:136-189), one launch for both images
//                         (blockIdx.z); the uint8 tile plus its halo is staged in LDS up to kLdsHalf, read from global memory
//                         above that — the same arithmetic in the same order either way.
//   dense_flow_kernel     the per-pixel Gauss-Newton refinement (:191-245), one pixel per lane; the initial flow is zero (coarsest
//                         level), the caller's planes (single-level overload) or the coarser level's smoothed flow upsampled in
//                         place (:66-77 — fused here, it is the same Interpolate(.) * 2.0f per pixel).
//   dense_median_kernel   SmoothFlow (:334-371): the 3x3 median of both planes under a total order.
// Every sum has a fixed, short, per-pixel order; with -ffp-contract=off and correctly rounded division / sqrt the results are
// bit-identical to the scalar restatement (tests/dense_flow_ref.c).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ftk_device.h"

namespace ftk {
namespace {

constexpr int kTile = 16;     // 16 x 16 pixels per workgroup (4 waves of 4 rows x 16 columns)
constexpr int kLdsHalf = 16;  // largest half patch whose tile + halo is staged in LDS
constexpr int kLdsSide = kTile + 2 * kLdsHalf;
constexpr int kLdsWeights = (2 * kLdsHalf + 1) * (2 * kLdsHalf + 1);

// static_cast<int32_t>(float) as x86-64 cvttss2si (out of range / NaN -> INT_MIN), DESIGN.md section 2
__device__ __forceinline__ int f2i_x86(float x) { return (x >= -2147483648.0f && x < 2147483648.0f) ? (int)x : INT_MIN; }
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Utility::Interpolate(Mat, r, c): clamp-to-edge bilinear.  Taps and weights are shared by the six
// moment planes of one sample.
struct Taps {
    size_t i00, i01, i10, i11;
    float w00, w01, w10, w11;
};

__device__ __forceinline__ Taps make_taps(int rows, int cols, float r, float c) {
    const float fr = floorf(r), fc = floorf(c);
    const float sr = r - fr, sc = c - fc;
    const int r0i = f2i_x86(fr), c0i = f2i_x86(fc);
    const int r1i = (int)((unsigned)r0i + 1u), c1i = (int)((unsigned)c0i + 1u);
    const int r0 = clampi(r0i, 0, rows - 1), r1 = clampi(r1i, 0, rows - 1);
    const int c0 = clampi(c0i, 0, cols - 1), c1 = clampi(c1i, 0, cols - 1);
    Taps t;
    t.i00 = (size_t)r0 * (unsigned)cols + (unsigned)c0;
    t.i01 = (size_t)r0 * (unsigned)cols + (unsigned)c1;
    t.i10 = (size_t)r1 * (unsigned)cols + (unsigned)c0;
    t.i11 = (size_t)r1 * (unsigned)cols + (unsigned)c1;
    t.w00 = (1.0f - sr) * (1.0f - sc);
    t.w01 = (1.0f - sr) * sc;
    t.w10 = sr * (1.0f - sc);
    t.w11 = sr * sc;
    return t;
}

__device__ __forceinline__ float blend(const Taps &t, float tl, float tr, float bl, float br) {
    return ((tl * t.w00 + tr * t.w01) + bl * t.w10) + br * t.w11;
}

struct Coeffs {
    float a00, a01, a11, b0, b1;
};

// ConstructConstrainFunctionForPixel (:247-303 / :305-332): the literal expression order
__device__ __forceinline__ Coeffs coefficients(float S0, float Sr, float Sc, float Src, float Srr, float Scc, float k2, float k4, float k22) {
    const float D = k4 - k2 * k2;
    const float E = k22 - k2 * k2;
    const float inv_D_plus_E = 1.0f / (D + E + 1e-6f);
    const float inv_D_minus_E = 1.0f / (D - E + 1e-6f);
    const float term1 = (Srr + Scc - 2.0f * k2 * S0) * inv_D_plus_E;
    const float term2 = (Srr - Scc) * inv_D_minus_E;
    const float c_coeff = Src / (k22 + 1e-6f);
    Coeffs o;
    o.a00 = 0.5f * (term1 + term2);
    o.a11 = 0.5f * (term1 - term2);
    o.a01 = 0.5f * c_coeff;
    o.b0 = Sr / (k2 + 1e-6f);
    o.b1 = Sc / (k2 + 1e-6f);
    return o;
}

// The six moments of one pixel (:155-183): dr outer, dc inner, each term multiplied left to right, accumulators from 0.0f.
// fetch(dr, dc) returns the replicate-clamped pixel value, weight(dr, dc) the normalised Gaussian weight.
template <typename Fetch, typename Weight>
__device__ __forceinline__ void accumulate(int half, Fetch fetch, Weight weight, float4 &m0, float4 &m1) {
    float s0 = 0.0f, sr = 0.0f, sc = 0.0f, src = 0.0f, srr = 0.0f, scc = 0.0f;
    for (int dr = -half; dr <= half; ++dr) {
        const float fdr = (float)dr, fdr2 = (float)(dr * dr);
        for (int dc = -half; dc <= half; ++dc) {
            const float w = weight(dr, dc);
            const float val = fetch(dr, dc);
            s0 += val * w;
            sr += fdr * val * w;
            sc += (float)dc * val * w;
            src += (float)(dr * dc) * val * w;
            srr += fdr2 * val * w;
            scc += (float)(dc * dc) * val * w;
        }
    }
    m0 = make_float4(s0, sr, sc, src);
    m1 = make_float4(srr, scc, 0.0f, 0.0f);
}

template <bool kLds>
__global__ void __launch_bounds__(kTile *kTile) dense_moments_kernel(DenseMomentsParams p) {
    const int which = blockIdx.z;  // 0 = ref, 1 = cur
    const DevImage img = p.img[which];
    if ((int)blockIdx.y * kTile >= img.rows || (int)blockIdx.x * kTile >= img.cols) {
        return;  // the grid covers the larger of the two images (uniform per workgroup: before any barrier)
    }
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    const int row = blockIdx.y * kTile + ty, col = blockIdx.x * kTile + tx;
    const int half = p.half;
    const int size = 2 * half + 1;
    float4 m0, m1;
    if constexpr (kLds) {
        __shared__ float tile[kLdsSide * kLdsSide];
        __shared__ float wts[kLdsWeights];
        const int side = kTile + 2 * half;
        const int r_base = blockIdx.y * kTile - half, c_base = blockIdx.x * kTile - half;
        for (int k = threadIdx.x; k < side * side; k += kTile * kTile) {
            const int r = clampi(r_base + k / side, 0, img.rows - 1), c = clampi(c_base + k % side, 0, img.cols - 1);
            tile[k] = (float)img.data[(size_t)r * (unsigned)img.cols + (unsigned)c];
        }
        for (int k = threadIdx.x; k < size * size; k += kTile * kTile) {
            wts[k] = p.weights[k];
        }
        __syncthreads();
        if (row >= img.rows || col >= img.cols) {
            return;
        }
        // Inside the tile the clamp is already applied: the halo cell of (ty + dr, tx + dc) holds pixel (clamp(row + dr), clamp(col + dc)).
        const float *centre = tile + (ty + half) * side + (tx + half);
        const float *wc = wts + half * size + half;
        accumulate(half, [&](int dr, int dc) { return centre[dr * side + dc]; }, [&](int dr, int dc) { return wc[dr * size + dc]; }, m0, m1);
    } else {
        if (row >= img.rows || col >= img.cols) {
            return;
        }
        const float *wc = p.weights + (size_t)half * size + half;
        accumulate(
            half,
            [&](int dr, int dc) {
                const int r = clampi(row + dr, 0, img.rows - 1), c = clampi(col + dc, 0, img.cols - 1);
                return (float)img.data[(size_t)r * (unsigned)img.cols + (unsigned)c];
            },
            [&](int dr, int dc) { return wc[dr * size + dc]; }, m0, m1);
    }
    float4 *out = p.mom[which] + 2 * ((size_t)row * (unsigned)img.cols + (unsigned)col);
    out[0] = m0;
    out[1] = m1;
}

__global__ void __launch_bounds__(kTile *kTile) dense_flow_kernel(DenseFlowParams p) {
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    const int row = blockIdx.y * kTile + ty, col = blockIdx.x * kTile + tx;
    if (row >= p.ref_rows || col >= p.ref_cols) {
        return;
    }
    const size_t i = (size_t)row * (unsigned)p.ref_cols + (unsigned)col;
    const float k2 = p.k2, k4 = p.k4, k22 = p.k22;
    // reference side at the integer pixel (:195-197; the integer overload reads the moments directly)
    const float4 r0 = p.mom_ref[2 * i], r1 = p.mom_ref[2 * i + 1];
    const Coeffs c1 = coefficients(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, k2, k4, k22);
    float flow_r = 0.0f, flow_c = 0.0f;
    if (p.init == 1) {
        // single-level overload: a ref-sized plane is the initial guess, any other was reset to zero (:18-23)
        if (p.flow_valid & 1) {
            flow_r = p.init_r[i];
        }
        if (p.flow_valid & 2) {
            flow_c = p.init_c[i];
        }
    } else if (p.init == 2) {
        // the coarser level's smoothed flow, upsampled (:71-75)
        const Taps t = make_taps(p.init_rows, p.init_cols, (float)row * 0.5f, (float)col * 0.5f);
        flow_r = blend(t, p.init_r[t.i00], p.init_r[t.i01], p.init_r[t.i10], p.init_r[t.i11]) * 2.0f;
        flow_c = blend(t, p.init_c[t.i00], p.init_c[t.i01], p.init_c[t.i10], p.init_c[t.i11]) * 2.0f;
    }
    for (int iter = 0; iter < p.max_iteration; ++iter) {
        const float sample_r = (float)row + flow_r;  // :206-207
        const float sample_c = (float)col + flow_c;
        // :307-312: the six moments interpolated, then the same formula (never A / b interpolated)
        const Taps t = make_taps(p.cur_rows, p.cur_cols, sample_r, sample_c);
        const float4 a0 = p.mom_cur[2 * t.i00], a1 = p.mom_cur[2 * t.i00 + 1];
        const float4 b0 = p.mom_cur[2 * t.i01], b1 = p.mom_cur[2 * t.i01 + 1];
        const float4 e0 = p.mom_cur[2 * t.i10], e1 = p.mom_cur[2 * t.i10 + 1];
        const float4 d0 = p.mom_cur[2 * t.i11], d1 = p.mom_cur[2 * t.i11 + 1];
        const Coeffs c2 = coefficients(blend(t, a0.x, b0.x, e0.x, d0.x), blend(t, a0.y, b0.y, e0.y, d0.y), blend(t, a0.z, b0.z, e0.z, d0.z),
                                       blend(t, a0.w, b0.w, e0.w, d0.w), blend(t, a1.x, b1.x, e1.x, d1.x), blend(t, a1.y, b1.y, e1.y, d1.y), k2, k4, k22);
        // :215-220 A_avg = (A1 + A2) * 0.5f, M = A_avg * 2.0f (symmetric), b_diff = b1 - b2
        const float M00 = ((c1.a00 + c2.a00) * 0.5f) * 2.0f;
        const float M01 = ((c1.a01 + c2.a01) * 0.5f) * 2.0f;
        const float M10 = M01;
        const float M11 = ((c1.a11 + c2.a11) * 0.5f) * 2.0f;
        const float bd0 = c1.b0 - c2.b0, bd1 = c1.b1 - c2.b1;
        // :221-222 MtM = M^T M, Mtb = M^T b_diff
        const float T00 = M00 * M00 + M10 * M10, T01 = M00 * M01 + M10 * M11;
        const float T10 = M01 * M00 + M11 * M10, T11 = M01 * M01 + M11 * M11;
        const float g0 = M00 * bd0 + M10 * bd1, g1 = M01 * bd0 + M11 * bd1;
        // :225-226 lambda = 0.1 trace + 1, H = MtM + I * lambda (the off-diagonal gets + 0 * lambda)
        const float lambda = 0.1f * (T00 + T11) + 1.0f;
        const float H00 = T00 + 1.0f * lambda, H01 = T01 + 0.0f * lambda;
        const float H10 = T10 + 0.0f * lambda, H11 = T11 + 1.0f * lambda;
        // :227 H.inverse() (Eigen's 2x2 closed form) * Mtb
        const float invdet = 1.0f / (H00 * H11 - H10 * H01);
        const float I00 = H11 * invdet, I01 = -H01 * invdet, I10 = -H10 * invdet, I11 = H00 * invdet;
        float dr = I00 * g0 + I01 * g1;
        float dc = I10 * g0 + I11 * g1;
        // :230-234 step cap
        const float step_norm = sqrtf(dr * dr + dc * dc);
        if (step_norm > p.max_step) {
            const float s = p.max_step / step_norm;
            dr *= s;
            dc *= s;
        }
        flow_r += dr;  // :237-238
        flow_c += dc;
        if (dr * dr + dc * dc < p.converge) {  // :241
            break;
        }
    }
    p.out_r[i] = flow_r;
    p.out_c[i] = flow_c;
}

// Total-order key: -0 < +0, every NaN above +inf; signed integer compares, no dynamic indexing.
__device__ __forceinline__ int order_key(float v) {
    const int b = __float_as_int(v);
    return (v != v) ? INT_MAX : (b < 0 ? (b ^ 0x7FFFFFFF) : b);
}
__device__ __forceinline__ float key_value(int k) { return __int_as_float(k < 0 ? (k ^ 0x7FFFFFFF) : k); }

#define DF_SORT(a, b)              \
    {                              \
        const int lo_ = min(a, b); \
        b = max(a, b);             \
        a = lo_;                   \
    }
// Median of nine by a 19-exchange network (the 5th smallest; checked on all 2^9 0/1 inputs).
__device__ __forceinline__ int median9(int p0, int p1, int p2, int p3, int p4, int p5, int p6, int p7, int p8) {
    DF_SORT(p1, p2) DF_SORT(p4, p5) DF_SORT(p7, p8) DF_SORT(p0, p1) DF_SORT(p3, p4) DF_SORT(p6, p7) DF_SORT(p1, p2) DF_SORT(p4, p5)
    DF_SORT(p7, p8) DF_SORT(p0, p3) DF_SORT(p5, p8) DF_SORT(p4, p7) DF_SORT(p3, p6) DF_SORT(p1, p4) DF_SORT(p2, p5) DF_SORT(p4, p7)
    DF_SORT(p4, p2) DF_SORT(p6, p4) DF_SORT(p4, p2) return p4;
}
#undef DF_SORT

__device__ __forceinline__ float median_at(const float *plane, int cols, int rm, int r, int rp, int cm, int c, int cp) {
    const size_t a = (size_t)rm * (unsigned)cols, b = (size_t)r * (unsigned)cols, d = (size_t)rp * (unsigned)cols;
    return key_value(median9(order_key(plane[a + cm]), order_key(plane[a + c]), order_key(plane[a + cp]), order_key(plane[b + cm]), order_key(plane[b + c]),
                             order_key(plane[b + cp]), order_key(plane[d + cm]), order_key(plane[d + c]), order_key(plane[d + cp])));
}

__global__ void __launch_bounds__(kTile *kTile) dense_median_kernel(DenseMedianParams p) {
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    const int row = blockIdx.y * kTile + ty, col = blockIdx.x * kTile + tx;
    if (row >= p.rows || col >= p.cols) {
        return;
    }
    const int rm = max(row - 1, 0), rp = min(row + 1, p.rows - 1), cm = max(col - 1, 0), cp = min(col + 1, p.cols - 1);
    const size_t i = (size_t)row * (unsigned)p.cols + (unsigned)col;
    p.out_r[i] = median_at(p.in_r, p.cols, rm, row, rp, cm, col, cp);
    p.out_c[i] = median_at(p.in_c, p.cols, rm, row, rp, cm, col, cp);
}

dim3 tiles(int rows, int cols) { return dim3((unsigned)((cols + kTile - 1) / kTile), (unsigned)((rows + kTile - 1) / kTile)); }

}  // namespace

int dense_lds_half() { return kLdsHalf; }

hipError_t dense_moments_launch(const DenseMomentsParams &p, hipStream_t stream) {
    const int rows = p.img[0].rows > p.img[1].rows ? p.img[0].rows : p.img[1].rows;
    const int cols = p.img[0].cols > p.img[1].cols ? p.img[0].cols : p.img[1].cols;
    dim3 grid = tiles(rows, cols);
    grid.z = 2;
    if (p.half <= kLdsHalf) {
        hipLaunchKernelGGL(dense_moments_kernel<true>, grid, dim3(kTile * kTile), 0, stream, p);
    } else {
        hipLaunchKernelGGL(dense_moments_kernel<false>, grid, dim3(kTile * kTile), 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t dense_flow_launch(const DenseFlowParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(dense_flow_kernel, tiles(p.ref_rows, p.ref_cols), dim3(kTile * kTile), 0, stream, p);
    return hipGetLastError();
}

hipError_t dense_median_launch(const DenseMedianParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(dense_median_kernel, tiles(p.rows, p.cols), dim3(kTile * kTile), 0, stream, p);
    return hipGetLastError();
}

__global__ void dense_warm_kernel() {}
hipError_t dense_warm(hipStream_t stream) {
    hipLaunchKernelGGL(dense_warm_kernel, dim3(1), dim3(64), 0, stream);
    return hipGetLastError();
}

}  // namespace ftk
