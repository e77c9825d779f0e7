// raft_math.h — the device functions the RAFT kernels share: exp_c and, built on it, sigmoid_c and tanh_c
// (DESIGN.md 5.13).  Each is a stated sequence of correctly rounded float32 operations (the fused ones written as fmaf; the
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
