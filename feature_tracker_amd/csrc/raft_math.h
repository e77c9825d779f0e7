// raft_math.h — the device functions the RAFT kernels share: exp_c and, built on it, sigmoid_c and tanh_c
// (DESIGN.md 5.13), log_c (5.23) and erf_c (5.24).  Each is a stated sequence of correctly rounded float32 operations (the fused ones written as fmaf; the
// library is compiled with -ffp-contract=off), so a kernel that uses them can be held bit-identical to a scalar restatement.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ftk {

constexpr float kExpCutoff = -87.0f;
constexpr float kExpLog2e = 0x1.715476p+0f;
constexpr float kExpLn2Hi = 0x1.62e4p-1f;
constexpr float kExpLn2Lo = 0x1.7f7d1cp-20f;
constexpr float kTanhSmall = 0.25f;  // below it tanh_c is an odd polynomial

// exp_c of DESIGN.md 5.12, t <= 0 or NaN.
__device__ __forceinline__ float exp_c(float t) {
    if (t != t) {
        return t;
    }
    if (t < kExpCutoff) {
        return 0.0f;
    }
    const float n = rintf(t * kExpLog2e);
    float r = fmaf(n, -kExpLn2Hi, t);
    r = fmaf(n, -kExpLn2Lo, r);
    float p = 0x1.a01a02p-13f;
    p = fmaf(p, r, 0x1.6c16c2p-10f);
    p = fmaf(p, r, 0x1.111112p-7f);
    p = fmaf(p, r, 0x1.555556p-5f);
    p = fmaf(p, r, 0x1.555556p-3f);
    p = fmaf(p, r, 0x1p-1f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    return p * __uint_as_float((uint32_t)((int)n + 127) << 23);
}

constexpr uint32_t kLogSqrtHalfBits = 0x3f3504f3u;  // sqrt(1/2)
constexpr float kLogLn2Hi = 0x1.62e3p-1f;           // 0x3f317180: 16 significant bits, so k * kLogLn2Hi is exact for |k| < 256
constexpr float kLogLn2Lo = 0x1.2fefa2p-17f;        // 0x3717f7d1

// log_c of DESIGN.md 5.23, x a positive normal number or NaN (here x in [1, 4096]): x = 2^k m with m in [sqrt(1/2), sqrt(2)) taken
// off the bit pattern, f = m - 1 (exact), s = f / (2 + f), log m = 2 atanh(s) = f - f^2 / 2 + s (f^2 / 2 + R(s^2)) with R the four
// minimax coefficients of fdlibm's logf.  log_c(1) = +0; NaN gives NaN.
__device__ __forceinline__ float log_c(float x) {
    if (x != x) {
        return x;
    }
    const uint32_t ix = __float_as_uint(x) + (0x3f800000u - kLogSqrtHalfBits);
    const float dk = (float)((int)(ix >> 23) - 127);
    const float f = __fsub_rn(__uint_as_float((ix & 0x007fffffu) + kLogSqrtHalfBits), 1.0f);
    const float s = __fdiv_rn(f, __fadd_rn(2.0f, f));
    const float z = __fmul_rn(s, s);
    const float w = __fmul_rn(z, z);
    const float t1 = __fmul_rn(w, fmaf(w, 0x1.f13c4cp-3f, 0x1.999c26p-2f));
    const float t2 = __fmul_rn(z, fmaf(w, 0x1.23d3dcp-2f, 0x1.555554p-1f));
    const float R = __fadd_rn(t2, t1);
    const float hfsq = __fmul_rn(__fmul_rn(0.5f, f), f);
    float r = fmaf(s, __fadd_rn(hfsq, R), __fmul_rn(dk, kLogLn2Lo));
    r = __fadd_rn(__fsub_rn(r, hfsq), f);
    return fmaf(dk, kLogLn2Hi, r);
}

// ls of DESIGN.md 5.23 (log sigmoid): min(z, 0) - log_c(1 + exp_c(-|z|)); NaN gives NaN.
__device__ __forceinline__ float log_sigmoid_c(float z) {
    return __fsub_rn(fminf(z, 0.0f), log_c(__fadd_rn(1.0f, exp_c(-fabsf(z)))));
}

// erf_c of DESIGN.md 5.24; a = |x|.  a < 1: x P(x^2), P the Taylor coefficients 2 / sqrt(pi) (-1)^n / (n! (2 n + 1)) up to n = 12.
// 1 <= a < 4: 1 - exp_c(-(a a)) Q(1 / a), Q a degree-9 fit of erfc(a) exp(a^2) on [1, 4], with the sign of x.  a >= 4: +-1.  Odd,
// erf_c(+-0) = +-0, NaN gives NaN.
__device__ __forceinline__ float erf_c(float x) {
    if (x != x) {
        return x;
    }
    const float a = fabsf(x);
    if (a < 1.0f) {
        const float s = __fmul_rn(x, x);
        float p = 0x1.9e6ad6p-34f;
        p = fmaf(p, s, -0x1.51d718p-30f);
        p = fmaf(p, s, 0x1.fcc572p-27f);
        p = fmaf(p, s, -0x1.5f742ep-23f);
        p = fmaf(p, s, 0x1.b9e6cap-20f);
        p = fmaf(p, s, -0x1.f4d25cp-17f);
        p = fmaf(p, s, 0x1.f9a326p-14f);
        p = fmaf(p, s, -0x1.c02db4p-11f);
        p = fmaf(p, s, 0x1.565bcep-8f);
        p = fmaf(p, s, -0x1.b82ce4p-6f);
        p = fmaf(p, s, 0x1.ce2f22p-4f);
        p = fmaf(p, s, -0x1.812746p-2f);
        p = fmaf(p, s, 0x1.20dd76p+0f);
        return __fmul_rn(x, p);
    }
    if (a >= 4.0f) {
        return copysignf(1.0f, x);
    }
    const float t = __fdiv_rn(1.0f, a);
    float q = 0x1.eb6cf6p-6f;
    q = fmaf(q, t, -0x1.6687c8p-3f);
    q = fmaf(q, t, 0x1.b39f5p-2f);
    q = fmaf(q, t, -0x1.08bcdap-1f);
    q = fmaf(q, t, 0x1.c0ff9ap-3f);
    q = fmaf(q, t, 0x1.effe7ap-3f);
    q = fmaf(q, t, -0x1.85acaap-2f);
    q = fmaf(q, t, 0x1.634f56p-6f);
    q = fmaf(q, t, 0x1.1f8b32p-1f);
    q = fmaf(q, t, 0x1.11b274p-13f);
    const float e = exp_c(-__fmul_rn(a, a));
    return copysignf(__fsub_rn(1.0f, __fmul_rn(e, q)), x);
}

// sigmoid_c of DESIGN.md 5.13: 1 / (1 + e) for v >= 0 and e / (1 + e) otherwise, e = exp_c(-|v|); NaN gives NaN.
__device__ __forceinline__ float sigmoid_c(float v) {
    const float e = exp_c(-fabsf(v));
    const float d = __fadd_rn(1.0f, e);
    return v >= 0.0f ? __fdiv_rn(1.0f, d) : __fdiv_rn(e, d);
}

// tanh_c of DESIGN.md 5.13: |v| < 0.25: a + a * (s * P(s)), a = |v|, s = v * v, P the Taylor coefficients of tanh(x) / x - 1 up to x^10;
// otherwise (1 - e) / (1 + e), e = exp_c(-2 |v|), with the sign of v.  tanh_c(+-0) = +-0, NaN gives NaN.
__device__ __forceinline__ float tanh_c(float v) {
    const float a = fabsf(v);
    if (a < kTanhSmall) {
        const float s = __fmul_rn(v, v);
        float p = -0x1.226e36p-7f;
        p = fmaf(p, s, 0x1.664f48p-6f);
        p = fmaf(p, s, -0x1.ba1ba2p-5f);
        p = fmaf(p, s, 0x1.111112p-3f);
        p = fmaf(p, s, -0x1.555556p-2f);
        return copysignf(fmaf(a, __fmul_rn(s, p), a), v);
    }
    const float e = exp_c(__fmul_rn(-2.0f, a));
    const float t = __fdiv_rn(__fsub_rn(1.0f, e), __fadd_rn(1.0f, e));
    return copysignf(t, v);
}

}  // namespace ftk
