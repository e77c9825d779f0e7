// pnp_kernels.hip — PnpRansac on gfx950: the camera pose from landmarks and the pixels where they are seen, RANSAC over the
// six-point DLT and a Gauss-Newton refit of the reprojection error on the inliers, everything on the device, 5 + 2 refine_iterations
// launches of fixed shape.
//
//  * pnp_scan_kernel: the filters' scan (epipolar_device.h's ep_scan_participants_if: ONE workgroup lists the participants in ascending
//    index order) with this stage's test of a participant: status TRACKED, five finite numbers, a landmark other than (0, 0, 0).  It
//    stores the calibrated pixel and the landmark.
//  * pnp_hypothesis_kernel: one lane = one hypothesis, as two_view_hypothesis_kernel.  The six landmarks are conditioned from the sample
//    alone; the 11 x 12 DLT system lives in LDS, [entry][lane] (156 floats per lane, 39 KB per workgroup: complete pivoting indexes rows
//    and columns at run time), and the elimination is epipolar_device.h's ep_null_vector_of<11>, the two filters' at another size.
//  * pnp_p3p_hypothesis_kernel: the "p3p" sampler's kernel in the place of pnp_hypothesis_kernel: four participants,
//    Grunert's quartic by Ferrari's factorisation on the first three, the fourth chooses among the solutions; registers alone, no LDS.
//    Both hypothesis kernels begin with pnp_draw_sample and end with epipolar_device.h's ep_store_hypothesis.
//  * pnp_score_kernel: epipolar_device.h's ep_score_walk (a tile of 256 participants in LDS, 4 hypotheses per wave, ballot and popcount,
//    ONE integer atomicAdd per workgroup and hypothesis) on a participant record of five floats and a model of twelve, which is why it is
//    a kernel of its own and no third Model of the two-view family: the family's record is one float4 and its models are nine floats.
//  * pnp_select_kernel: ONE workgroup takes the winner key (epipolar_device.h's ep_winner_keys); thread 0 turns the winner's [A | b] into
//    a pose: the nearest rotation by pose_device.h's jacobi_eigen<3, Jacobi::Thread> on A^T A (one thread on LDS arrays: the other
//    threads have returned), the quaternion by pose_quaternion_of_transpose.
//  * pnp_sums_kernel / pnp_step_kernel, once per refit step: a tile of 256 participants reduces its 27 terms by pose_device.h's
//    pose_tree_sum (the first step over the inliers of the model that won, the later ones over the current pose's) and counts them by
//    pose_block_counts; one wave adds the tile totals in tile order (pose_tile_total), solves the 6 x 6 system by an LDL^T and moves the
//    pose, or ends the refit.
//  * pnp_finish_kernel: a thread per participant applies the status rule under the final pose (pose_block_counts_add counts the
//    inliers); block 0 writes the outputs.
// Every float operation below is stated in DESIGN.md 5.30 and restated in tests/pnp_ref.c; the build has no contraction (-ffp-contract=off)
// and correctly rounded division and square root.
#include "pnp_plan.h"
#include "pose_device.h"

namespace ftk {
namespace {

constexpr int kFlagOk = 0, kFlagDone = 1, kFlagWinner = 2;

__global__ void __launch_bounds__(kEpipolarScanBlock) pnp_scan_kernel(const PnpParams p) {
    __shared__ int32_t scan[kEpipolarScanBlock];
    ep_scan_participants_if(
        scan, p.n, p.scan_per_thread, p.m,
        [&](const int i) {
            if (p.status[i] != FTK_TRACKED) {
                return false;  // (nothing else of a point that is not TRACKED is read)
            }
            const float X = p.landmarks[3 * (size_t)i], Y = p.landmarks[3 * (size_t)i + 1], Z = p.landmarks[3 * (size_t)i + 2];
            const float2 c = reinterpret_cast<const float2 *>(p.uv)[i];
            return ep_finite(X) && ep_finite(Y) && ep_finite(Z) && ep_finite(c.x) && ep_finite(c.y) && !(X == 0.0f && Y == 0.0f && Z == 0.0f);
        },
        [&](const int at, const int i) {
            const float X = p.landmarks[3 * (size_t)i], Y = p.landmarks[3 * (size_t)i + 1], Z = p.landmarks[3 * (size_t)i + 2];
            const float2 c = reinterpret_cast<const float2 *>(p.uv)[i];
            p.points[at] = make_float4((c.x - p.cx) / p.fx, (c.y - p.cy) / p.fy, X, Y);
            p.depth[at] = Z;
            p.list[at] = i;
        });
}

// The head of a hypothesis kernel: hypothesis h's draw of S participants and their (x, y, X, Y, Z), zeros when the draw failed.
template <int S>
__device__ __forceinline__ bool pnp_draw_sample(const PnpParams &p, const int h, uint32_t (&idx)[S], float (&x)[S], float (&y)[S], float (&X)[S],
                                                float (&Y)[S], float (&Z)[S]) {
    const uint32_t m = (uint32_t)max(min(p.m[0], p.n), 0);
    const bool ok = ep_draw<S>(p.seed, (uint32_t)h, m, idx);
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const float4 q = ok ? p.points[idx[k]] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        x[k] = q.x, y[k] = q.y, X[k] = q.z, Y[k] = q.w;
        Z[k] = ok ? p.depth[idx[k]] : 0.0f;
    }
    return ok;
}

__global__ void __launch_bounds__(kEpipolarHypBlock) pnp_hypothesis_kernel(const PnpParams p) {
    __shared__ float lds[kPnpHypLdsFloats * kEpipolarHypBlock];
    const int lane = threadIdx.x;
    const int h = blockIdx.x * kEpipolarHypBlock + lane;
    if (h >= p.hypotheses) {
        return;  // (no barrier below)
    }
    constexpr int L = kEpipolarHypBlock, C = kPnpRows + 1;
    float *const a = lds + lane;                                                // a[(r * 12 + c) * 64]
    int *const perm = reinterpret_cast<int *>(lds + kPnpRows * C * L) + lane;   // perm[c * 64]
    float *const fv = lds + (kPnpRows * C + C) * L + lane;                      // fv[c * 64]
    uint32_t idx[kPnpSample];
    float x[kPnpSample], y[kPnpSample], X[kPnpSample], Y[kPnpSample], Z[kPnpSample];
    bool ok = pnp_draw_sample(p, h, idx, x, y, X, Y, Z);
    // conditioning from the sample alone: the mean in index order, the mean absolute deviation over the 18 coordinates
    const float mx = (((((X[0] + X[1]) + X[2]) + X[3]) + X[4]) + X[5]) / 6.0f;
    const float my = (((((Y[0] + Y[1]) + Y[2]) + Y[3]) + Y[4]) + Y[5]) / 6.0f;
    const float mz = (((((Z[0] + Z[1]) + Z[2]) + Z[3]) + Z[4]) + Z[5]) / 6.0f;
    float dev = 0.0f;
#pragma unroll
    for (int k = 0; k < kPnpSample; ++k) {
        X[k] = X[k] - mx, Y[k] = Y[k] - my, Z[k] = Z[k] - mz;
        const float d = (fabsf(X[k]) + fabsf(Y[k])) + fabsf(Z[k]);
        dev = k == 0 ? d : dev + d;
    }
    const float s = dev / 18.0f;
    ok = ok && ep_finite(s) && s > 0.0f;
    if (ok) {
#pragma unroll
        for (int k = 0; k < kPnpSample; ++k) {
            const float Xn = X[k] / s, Yn = Y[k] / s, Zn = Z[k] / s;
            const int r0 = 2 * k * C, r1 = (2 * k + 1) * C;
            a[(r0 + 0) * L] = Xn;
            a[(r0 + 1) * L] = Yn;
            a[(r0 + 2) * L] = Zn;
            a[(r0 + 3) * L] = 1.0f;
            a[(r0 + 4) * L] = 0.0f;
            a[(r0 + 5) * L] = 0.0f;
            a[(r0 + 6) * L] = 0.0f;
            a[(r0 + 7) * L] = 0.0f;
            a[(r0 + 8) * L] = -(x[k] * Xn);
            a[(r0 + 9) * L] = -(x[k] * Yn);
            a[(r0 + 10) * L] = -(x[k] * Zn);
            a[(r0 + 11) * L] = -x[k];
            if (2 * k + 1 < kPnpRows) {  // (the twelfth row is not used)
                a[(r1 + 0) * L] = 0.0f;
                a[(r1 + 1) * L] = 0.0f;
                a[(r1 + 2) * L] = 0.0f;
                a[(r1 + 3) * L] = 0.0f;
                a[(r1 + 4) * L] = Xn;
                a[(r1 + 5) * L] = Yn;
                a[(r1 + 6) * L] = Zn;
                a[(r1 + 7) * L] = 1.0f;
                a[(r1 + 8) * L] = -(y[k] * Xn);
                a[(r1 + 9) * L] = -(y[k] * Yn);
                a[(r1 + 10) * L] = -(y[k] * Zn);
                a[(r1 + 11) * L] = -y[k];
            }
        }
    }
    float f[C];
    ok = ep_null_vector_of<kPnpRows, L>(a, perm, fv, ok, f);
    float P[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        P[i] = 0.0f;
    }
    if (ok) {
        // the conditioning folded back, times s: A = the normalised A, b = s b_n - A mean
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            P[r * 4] = f[r * 4], P[r * 4 + 1] = f[r * 4 + 1], P[r * 4 + 2] = f[r * 4 + 2];
            P[r * 4 + 3] = s * f[r * 4 + 3] - ((f[r * 4] * mx + f[r * 4 + 1] * my) + f[r * 4 + 2] * mz);
        }
        // the sign: the sample's depths positive (X, Y, Z hold the centred landmarks: the sample is read again)
        int front = 0, behind = 0;
#pragma unroll
        for (int k = 0; k < kPnpSample; ++k) {
            const float4 q = p.points[idx[k]];
            const float w = ((P[8] * q.z + P[9] * q.w) + P[10] * p.depth[idx[k]]) + P[11];
            front += w > 0.0f ? 1 : 0;
            behind += w < 0.0f ? 1 : 0;
        }
        ok = front == kPnpSample || behind == kPnpSample;
        if (behind == kPnpSample) {
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                P[i] = -P[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            ok = ok && ep_finite(P[i]);
        }
    }
    ep_store_hypothesis(p.models, p.valid, p.counts, h, ok, P);
}

// ---- the "p3p" sampler (tests/pnp_p3p_ref.c states every operation below in the same order) ----

__device__ __forceinline__ void p3p_cross(const float (&a)[3], const float (&b)[3], float (&r)[3]) {
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ float p3p_dot(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// One Newton step on y^3 + r2 y^2 + r1 y + r0; a step that is not finite is not taken.
__device__ __forceinline__ float p3p_cubic_step(const float y, const float r2, const float r1, const float r0) {
    const float val = ((y + r2) * y + r1) * y + r0;
    const float der = (3.0f * y + 2.0f * r2) * y + r1;
    const float step = val / der;
    return ep_finite(step) ? y - step : y;
}

// What three participants fix before any root is known: the bearings f and their cosines, the landmarks' frame (d01, d02, n = d01 x d02,
// nn = |n|^2), the squared sides a, b, c, u = N(w) / D(w), and the real roots w = s2 / s0 - 1 of Grunert's quartic in the slots of the two
// quadratics of Ferrari's factorisation (slots 0, 1 when pair[0], slots 2, 3 when pair[1]).
struct P3pSetup {
    float f[3][3];
    float c01, c02, c12;
    float d01[3], d02[3], n[3], nn;
    float a, b, c;
    float N[3], D[2], alpha2;
    float w[4];
    bool pair[2];
};

// false: the degeneracy test fired (two equal bearings, coincident or collinear landmarks, a leading coefficient of zero, not finite).
__device__ __forceinline__ bool p3p_setup(const float (&x)[4], const float (&y)[4], const float (&X)[4], const float (&Y)[4], const float (&Z)[4], P3pSetup &s) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float len = sqrtf((x[k] * x[k] + y[k] * y[k]) + 1.0f);
        s.f[k][0] = x[k] / len, s.f[k][1] = y[k] / len, s.f[k][2] = 1.0f / len;
    }
    s.c01 = p3p_dot(s.f[0], s.f[1]), s.c02 = p3p_dot(s.f[0], s.f[2]), s.c12 = p3p_dot(s.f[1], s.f[2]);
    float g1[3], g2[3], m[3], d12[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        g1[e] = s.f[1][e] - s.f[0][e], g2[e] = s.f[2][e] - s.f[0][e];
    }
    p3p_cross(g1, g2, m);
    const float mm = p3p_dot(m, m);
    bool ok = ep_finite(mm) && mm > 0.0f;
    s.d01[0] = X[1] - X[0], s.d01[1] = Y[1] - Y[0], s.d01[2] = Z[1] - Z[0];
    s.d02[0] = X[2] - X[0], s.d02[1] = Y[2] - Y[0], s.d02[2] = Z[2] - Z[0];
    d12[0] = X[2] - X[1], d12[1] = Y[2] - Y[1], d12[2] = Z[2] - Z[1];
    s.c = p3p_dot(s.d01, s.d01), s.b = p3p_dot(s.d02, s.d02), s.a = p3p_dot(d12, d12);
    p3p_cross(s.d01, s.d02, s.n);
    s.nn = p3p_dot(s.n, s.n);
    ok = ok && ep_finite(s.nn) && s.nn > 0.0f;
    // v = 1 + w: alpha = 1 - c02 and delta = c12 - c01 from differences of bearings
    const float alpha = 0.5f * p3p_dot(g2, g2), delta = p3p_dot(s.f[1], g2);
    const float B = s.a / s.b, k = (s.c - s.a) / s.b;
    const float n0 = 2.0f * (k * alpha), n1 = n0 + 2.0f, n2 = k + 1.0f;
    const float e0 = 2.0f * delta, e1 = 2.0f * s.c12;
    s.N[0] = n0, s.N[1] = n1, s.N[2] = n2, s.D[0] = e0, s.D[1] = e1, s.alpha2 = 2.0f * alpha;
    const float a2 = s.alpha2, t12 = 2.0f * s.c12;
    const float g0 = e0 * e0, g1c = 2.0f * (e0 * e1), g2c = e1 * e1;
    const float h0 = n0 * e0, h1 = n0 * e1 + n1 * e0, h2 = n1 * e1 + n2 * e0, h3 = n2 * e1;
    const float k4 = ((n2 * n2 + g2c) - t12 * h3) - B * g2c;
    const float k3 = ((2.0f * (n1 * n2) + (2.0f * g2c + g1c)) - t12 * (h3 + h2)) - B * (a2 * g2c + g1c);
    const float k2 = (((2.0f * (n0 * n2) + n1 * n1) + ((g2c + 2.0f * g1c) + g0)) - t12 * (h2 + h1)) - B * ((a2 * g2c + a2 * g1c) + g0);
    const float k1 = ((2.0f * (n0 * n1) + (g1c + 2.0f * g0)) - t12 * (h1 + h0)) - B * (a2 * g1c + a2 * g0);
    const float k0 = ((n0 * n0 + g0) - t12 * h0) - B * (a2 * g0);
    ok = ok && ep_finite(k4) && k4 != 0.0f;
    const float p3 = k3 / k4, p2 = k2 / k4, p1 = k1 / k4, p0 = k0 / k4;
    // Ferrari: the largest real root of the resolvent cubic, kP3pCubicSteps Newton steps from Cauchy's bound on the convex (concave) side
    const float r2 = -p2, r1 = p3 * p1 - 4.0f * p0, r0 = (4.0f * (p2 * p0) - (p3 * p3) * p0) - p1 * p1;
    float bound = fabsf(r2);
    if (fabsf(r1) > bound) {
        bound = fabsf(r1);
    }
    if (fabsf(r0) > bound) {
        bound = fabsf(r0);
    }
    const float xi = -r2 / 3.0f;
    const float at_xi = ((xi + r2) * xi + r1) * xi + r0;
    float yr = at_xi > 0.0f ? -(1.0f + bound) : 1.0f + bound;
    for (int i = 0; i < kP3pCubicSteps; ++i) {  // (a fixed count: no test of a float ends this loop)
        yr = p3p_cubic_step(yr, r2, r1, r0);
    }
    const float db = r2 + yr, dc = r1 + db * yr;
    const float ddisc = db * db - 4.0f * dc;
    if (ddisc >= 0.0f) {
        const float other = (-db + sqrtf(ddisc)) * 0.5f;
        if (other > yr) {
            yr = other;
        }
    }
#pragma unroll
    for (int i = 0; i < kP3pCubicPolish; ++i) {
        yr = p3p_cubic_step(yr, r2, r1, r0);
    }
    const float hp = 0.5f * p3, hy = 0.5f * yr;
    const float R2 = (hp * hp - p2) + yr, S2 = hy * hy - p0, RS = 0.5f * (hp * yr - p1);
    float R = 0.0f, S = 0.0f;
    if (R2 >= S2 && R2 > 0.0f) {
        R = sqrtf(R2), S = RS / R;
    } else if (S2 > 0.0f) {
        S = sqrtf(S2), R = RS / S;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float beta = j == 0 ? hp + R : hp - R, gamma = j == 0 ? hy + S : hy - S;
        const float disc = beta * beta - 4.0f * gamma;
        s.pair[j] = disc >= 0.0f;
        const float sq = sqrtf(s.pair[j] ? disc : 0.0f);
        s.w[2 * j] = (-beta + sq) * 0.5f;
        s.w[2 * j + 1] = (-beta - sq) * 0.5f;
    }
    return ok;
}

// The pose [R | t] of root w: the distances, kP3pNewtonSteps Newton steps on the three distance equations, the residual test, the two
// frames.  false: a distance is not positive, a residual is too large or an entry is not finite.
__device__ __forceinline__ bool p3p_pose(const P3pSetup &s, const float w, const float X0, const float Y0w, const float Z0, float (&P)[12]) {
    const float u = ((s.N[2] * w + s.N[1]) * w + s.N[0]) / (s.D[1] * w + s.D[0]);
    const float v = 1.0f + w;
    const float qv = (w * w + s.alpha2 * w) + s.alpha2;
    float s0 = sqrtf(s.b / qv), s1 = u * s0, s2 = v * s0;
#pragma unroll
    for (int i = 0; i < kP3pNewtonSteps; ++i) {
        const float q0 = ((s0 * s0 + s1 * s1) - (2.0f * s.c01) * (s0 * s1)) - s.c;
        const float q1 = ((s0 * s0 + s2 * s2) - (2.0f * s.c02) * (s0 * s2)) - s.b;
        const float q2 = ((s1 * s1 + s2 * s2) - (2.0f * s.c12) * (s1 * s2)) - s.a;
        const float j00 = 2.0f * (s0 - s1 * s.c01), j01 = 2.0f * (s1 - s0 * s.c01);
        const float j10 = 2.0f * (s0 - s2 * s.c02), j12 = 2.0f * (s2 - s0 * s.c02);
        const float j21 = 2.0f * (s1 - s2 * s.c12), j22 = 2.0f * (s2 - s1 * s.c12);
        const float det = -(j00 * (j12 * j21)) - j01 * (j10 * j22);
        const float m12 = q1 * j22 - j12 * q2;
        const float x0 = (-(q0 * (j12 * j21)) - j01 * m12) / det;
        const float x1 = (j00 * m12 - q0 * (j10 * j22)) / det;
        const float x2 = ((-(j00 * (q1 * j21)) - j01 * (j10 * q2)) + q0 * (j10 * j21)) / det;
        s0 = s0 - x0, s1 = s1 - x1, s2 = s2 - x2;
    }
    bool ok = s0 > 0.0f && s1 > 0.0f && s2 > 0.0f;
    {
        const float t0 = s0 * s0, t1 = s1 * s1, t2 = s2 * s2;
        const float q0 = ((t0 + t1) - (2.0f * s.c01) * (s0 * s1)) - s.c;
        const float q1 = ((t0 + t2) - (2.0f * s.c02) * (s0 * s2)) - s.b;
        const float q2 = ((t1 + t2) - (2.0f * s.c12) * (s1 * s2)) - s.a;
        ok = ok && fabsf(q0) <= kP3pResidual * (t0 + t1) && fabsf(q1) <= kP3pResidual * (t0 + t2) && fabsf(q2) <= kP3pResidual * (t1 + t2);
    }
    float C0[3], e1[3], e2[3], e3[3], i1[3], i2[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        C0[e] = s0 * s.f[0][e];
        e1[e] = s1 * s.f[1][e] - C0[e];
        e2[e] = s2 * s.f[2][e] - C0[e];
    }
    p3p_cross(e1, e2, e3);
    p3p_cross(s.d02, s.n, i1);
    p3p_cross(s.n, s.d01, i2);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            P[r * 4 + c] = ((e1[r] * i1[c] + e2[r] * i2[c]) + e3[r] * s.n[c]) / s.nn;
        }
        P[r * 4 + 3] = C0[r] - ((P[r * 4] * X0 + P[r * 4 + 1] * Y0w) + P[r * 4 + 2] * Z0);
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        ok = ok && ep_finite(P[i]);
    }
    return ok;
}

// One lane = one hypothesis: four participants, the first three to the solver, the fourth chooses among its solutions, which are formed
// and judged one at a time (one candidate and the best so far are live, never four poses).  No LDS.
__global__ void __launch_bounds__(kEpipolarHypBlock) pnp_p3p_hypothesis_kernel(const PnpParams p) {
    const int h = blockIdx.x * kEpipolarHypBlock + threadIdx.x;
    if (h >= p.hypotheses) {
        return;
    }
    uint32_t idx[kP3pSample];
    float x[kP3pSample], y[kP3pSample], X[kP3pSample], Y[kP3pSample], Z[kP3pSample];
    bool ok = pnp_draw_sample(p, h, idx, x, y, X, Y, Z);
    P3pSetup s;
    ok = p3p_setup(x, y, X, Y, Z, s) && ok;
    float P[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        P[i] = 0.0f;
    }
    bool have = false;
    float best = 0.0f;
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {  // the solutions in the order they are produced: w+ and w- of the first quadratic, then of the second
        const float w = i == 0 ? s.w[0] : i == 1 ? s.w[1] : i == 2 ? s.w[2] : s.w[3];
        float Q[12];
        bool take = ok && (i < 2 ? s.pair[0] : s.pair[1]) && p3p_pose(s, w, X[0], Y[0], Z[0], Q);
        float c[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < kP3pSample; ++k) {  // every sample point in front; c ends as the fourth point's camera coordinates
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                c[e] = ((Q[e * 4] * X[k] + Q[e * 4 + 1] * Y[k]) + Q[e * 4 + 2] * Z[k]) + Q[e * 4 + 3];
            }
            take = take && c[2] > 0.0f;
        }
        const float ex = c[0] - x[3] * c[2];
        const float ey = (c[1] - y[3] * c[2]) * p.ry;
        const float err = ex * ex + ey * ey;
        take = take && ep_finite(err) && (!have || err < best);
        if (take) {
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                P[e] = Q[e];
            }
            best = err, have = true;
        }
    }
    ep_store_hypothesis(p.models, p.valid, p.counts, h, have, P);
}

__global__ void __launch_bounds__(kEpipolarScoreTile) pnp_score_kernel(const PnpParams p) {
    __shared__ float4 tile[kEpipolarScoreTile];
    __shared__ float tile_z[kEpipolarScoreTile];
    ep_score_walk<12>(
        min(p.m[0], p.n), p.sample, p.hypotheses, p.models, p.valid, p.counts,
        [&](const int at, const int j, const bool live) {
            tile[at] = live ? p.points[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            tile_z[at] = live ? p.depth[j] : 0.0f;
        },
        [&](const float (&P)[12], const int at) {
            const float4 q = tile[at];
            const float Z = tile_z[at];
            float c[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                c[e] = ((P[e * 4] * q.z + P[e * 4 + 1] * q.w) + P[e * 4 + 2] * Z) + P[e * 4 + 3];
            }
            return pnp_inlier(c, q.x, q.y, p.ry, p.tn2);
        });
}

// The winner's P = [A | b] as a pose (q_rc, p_rc): R the nearest rotation to A, t = b / s with s the mean singular value; R_rc = R^T,
// p_rc = -R^T t.  M, V: 9 floats of LDS each.  false: singular or not finite.
__device__ __forceinline__ bool pnp_pose_of_model(const float (&P)[12], float *const M, float *const V, float (&ps)[7]) {
    float A[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            A[r * 3 + c] = P[r * 4 + c];
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            M[i * 3 + j] = (A[i] * A[j] + A[3 + i] * A[3 + j]) + A[6 + i] * A[6 + j];
        }
    }
    jacobi_eigen<3, Jacobi::Thread>(M, V, 0);
    const float l0 = M[0], l1 = M[4], l2 = M[8];
    if (!(l0 > 0.0f && l1 > 0.0f && l2 > 0.0f)) {
        return false;
    }
    const float sg0 = sqrtf(l0), sg1 = sqrtf(l1), sg2 = sqrtf(l2);
    const float det = (A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])) + A[2] * (A[3] * A[7] - A[4] * A[6]);
    if (!ep_finite(det) || det == 0.0f) {
        return false;
    }
    // det < 0: the term of the smallest eigenvalue (the lowest index among equals) enters with the other sign
    int small = 0;
    if (l1 < l0) {
        small = 1;
    }
    if (l2 < (small == 0 ? l0 : l1)) {
        small = 2;
    }
    float w0 = 1.0f / sg0, w1 = 1.0f / sg1, w2 = 1.0f / sg2;
    if (det < 0.0f) {
        w0 = small == 0 ? -w0 : w0, w1 = small == 1 ? -w1 : w1, w2 = small == 2 ? -w2 : w2;
    }
    // R = A W, W = V diag(w) V^T
    float W[9], R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            W[i * 3 + j] = ((V[i * 3] * w0) * V[j * 3] + (V[i * 3 + 1] * w1) * V[j * 3 + 1]) + (V[i * 3 + 2] * w2) * V[j * 3 + 2];
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            R[i * 3 + j] = (A[i * 3] * W[j] + A[i * 3 + 1] * W[3 + j]) + A[i * 3 + 2] * W[6 + j];
        }
    }
    const float sc = ((sg0 + sg1) + sg2) / 3.0f;
    const float t0 = P[3] / sc, t1 = P[7] / sc, t2 = P[11] / sc;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ps[4 + j] = -((R[j] * t0 + R[3 + j] * t1) + R[6 + j] * t2);
    }
    pose_quaternion_of_transpose(R, ps);  // R_rc = R^T
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        ok = ok && ep_finite(ps[e]);
    }
    return ok;
}

__global__ void __launch_bounds__(kEpipolarScanBlock) pnp_select_kernel(const PnpParams p) {
    __shared__ unsigned long long red[1][kEpipolarScanBlock];
    __shared__ float M[9], V[9];
    unsigned long long best[1];
    ep_winner_keys<1>(red, p.select_per_thread, p.hypotheses, best, [&](const int, const int h) { return p.counts[h]; });
    if (threadIdx.x != 0) {
        return;
    }
    const unsigned long long key = best[0];
    const int m = min(p.m[0], p.n);
    bool ok = m >= p.sample && ep_key_has_winner(key);  // (with fewer participants than a sample no hypothesis was formed)
    const int h = ok ? ep_key_hypothesis(key) : -1;
    float ps[7] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (ok) {
        float P[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            P[e] = p.models[(size_t)h * 12 + e];
        }
        ok = pnp_pose_of_model(P, M, V, ps);
    }
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        p.state[e] = ps[e];
    }
    p.state[7] = 0.0f;
    p.flags[kFlagOk] = ok ? 1 : 0;
    p.flags[kFlagDone] = ok ? 0 : 1;
    p.flags[kFlagWinner] = ok ? h : -1;
    p.flags[3] = 0;
    p.n_inliers[0] = 0;
}

__global__ void __launch_bounds__(kPoseTile) pnp_sums_kernel(const PnpParams p) {
    __shared__ float tree[kPnpSums][kPoseTile];
    __shared__ int32_t counts[1][kPoseTile / 64];
    const int m = min(p.m[0], p.n);
    const int base = blockIdx.x * kPoseTile;
    if (p.flags[kFlagOk] == 0 || p.flags[kFlagDone] != 0 || base >= m) {
        return;  // the whole workgroup: the grid covers n, the step kernel reads the tiles below M alone
    }
    const int tid = threadIdx.x;
    float ps[7], R[9];
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        ps[e] = p.state[e];
    }
    pnp_rotation(ps, R);
    bool in = false;
    float term[kPnpSums];
#pragma unroll
    for (int e = 0; e < kPnpSums; ++e) {
        term[e] = 0.0f;
    }
    if (base + tid < m) {
        const float4 q = p.points[base + tid];
        float c[3];
        const float Z = p.depth[base + tid];
        pnp_camera(R, ps, q.z, q.w, Z, c);
        if (p.step == 0) {  // the first step refits on the inliers of the model that won, those in front of the camera under the pose
            const float *const P = p.models + (size_t)p.flags[kFlagWinner] * 12;
            float cp[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                cp[e] = ((P[e * 4] * q.z + P[e * 4 + 1] * q.w) + P[e * 4 + 2] * Z) + P[e * 4 + 3];
            }
            in = pnp_inlier(cp, q.x, q.y, p.ry, p.tn2) && c[2] > 0.0f;
        } else {
            in = pnp_inlier(c, q.x, q.y, p.ry, p.tn2);
        }
        if (in) {
            const float ry = p.ry;
            const float iz = 1.0f / c[2];
            const float a = c[0] * iz, b = c[1] * iz;
            const float j1[6] = {a * b, -(1.0f + a * a), b, -iz, 0.0f, a * iz};
            const float j2[6] = {ry * (1.0f + b * b), ry * -(a * b), ry * -a, 0.0f, ry * -iz, ry * (b * iz)};
            const float r1 = a - q.x, r2 = (b - q.y) * ry;
            int e = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = i; j < 6; ++j, ++e) {
                    term[e] = j1[i] * j1[j] + j2[i] * j2[j];
                }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i, ++e) {
                term[e] = j1[i] * r1 + j2[i] * r2;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < kPnpSums; ++e) {
        tree[e][tid] = term[e];
    }
    const bool flags[1] = {in};
    pose_block_counts(counts, flags, [&](const int, const int32_t sum) { p.tile_counts[blockIdx.x] = sum; });  // (its barrier is the tree's)
    pose_tree_sum(tree, tid);
    if (tid < kPnpSums) {
        p.totals[(size_t)blockIdx.x * kPnpSums + tid] = tree[tid][0];
    }
}

__global__ void __launch_bounds__(kPoseSolveBlock) pnp_step_kernel(const PnpParams p) {
    __shared__ float sums[kPnpSums];
    __shared__ float H[36], Lm[36], d[6], y[6], dx[6];
    const int tid = threadIdx.x;
    if (p.flags[kFlagOk] == 0 || p.flags[kFlagDone] != 0) {
        return;  // the whole workgroup
    }
    const int m = min(p.m[0], p.n);
    const int tiles = (m + kPoseTile - 1) / kPoseTile;
    if (tid < kPnpSums) {
        sums[tid] = pose_tile_total(p.totals, tiles, kPnpSums, tid);
    }
    __syncthreads();
    if (tid != 0) {
        return;
    }
    int32_t count = 0;
    for (int t = 0; t < tiles; ++t) {
        count += p.tile_counts[t];
    }
    bool take = count >= kPnpRefitRows;
    if (take) {  // H x = -g by an LDL^T without pivoting, column by column
        int e = 0;
        for (int i = 0; i < 6; ++i) {
            for (int j = i; j < 6; ++j, ++e) {
                H[i * 6 + j] = sums[e];
                H[j * 6 + i] = sums[e];
            }
        }
        for (int j = 0; take && j < 6; ++j) {
            float acc = H[j * 6 + j];
            for (int k = 0; k < j; ++k) {
                acc = acc - (Lm[j * 6 + k] * Lm[j * 6 + k]) * d[k];
            }
            take = ep_finite(acc) && acc > 0.0f;
            d[j] = acc;
            for (int i = j + 1; take && i < 6; ++i) {
                float v = H[i * 6 + j];
                for (int k = 0; k < j; ++k) {
                    v = v - (Lm[i * 6 + k] * Lm[j * 6 + k]) * d[k];
                }
                Lm[i * 6 + j] = v / acc;
            }
        }
    }
    if (take) {
        for (int i = 0; i < 6; ++i) {
            float v = -sums[21 + i];
            for (int k = 0; k < i; ++k) {
                v = v - Lm[i * 6 + k] * y[k];
            }
            y[i] = v;
        }
        for (int i = 0; i < 6; ++i) {
            y[i] = y[i] / d[i];
        }
        for (int i = 5; i >= 0; --i) {
            float v = y[i];
            for (int k = i + 1; k < 6; ++k) {
                v = v - Lm[k * 6 + i] * dx[k];
            }
            dx[i] = v;
        }
        // q <- q (1, dtheta / 2), renormalised; p <- p + R_rc dt
        float ps[7], R[9];
#pragma unroll
        for (int e = 0; e < 7; ++e) {
            ps[e] = p.state[e];
        }
        pnp_rotation(ps, R);
        const float w = ps[0], x = ps[1], yq = ps[2], z = ps[3], hx = 0.5f * dx[0], hy = 0.5f * dx[1], hz = 0.5f * dx[2];
        float nq0 = ((w - x * hx) - yq * hy) - z * hz;
        float nq1 = ((x + w * hx) + yq * hz) - z * hy;
        float nq2 = ((yq + w * hy) + z * hx) - x * hz;
        float nq3 = ((z + w * hz) + x * hy) - yq * hx;
        const float qn = sqrtf(((nq0 * nq0 + nq1 * nq1) + nq2 * nq2) + nq3 * nq3);
        nq0 = nq0 / qn, nq1 = nq1 / qn, nq2 = nq2 / qn, nq3 = nq3 / qn;
        const float d3 = dx[3], d4 = dx[4], d5 = dx[5];
        const float np0 = ps[4] + ((R[0] * d3 + R[1] * d4) + R[2] * d5);
        const float np1 = ps[5] + ((R[3] * d3 + R[4] * d4) + R[5] * d5);
        const float np2 = ps[6] + ((R[6] * d3 + R[7] * d4) + R[8] * d5);
        take = ep_finite(nq0) && ep_finite(nq1) && ep_finite(nq2) && ep_finite(nq3) && ep_finite(np0) && ep_finite(np1) && ep_finite(np2);
        if (take) {
            p.state[0] = nq0, p.state[1] = nq1, p.state[2] = nq2, p.state[3] = nq3;
            p.state[4] = np0, p.state[5] = np1, p.state[6] = np2;
        }
    }
    if (!take) {
        p.flags[kFlagDone] = 1;  // the pose before this step stands
    }
}

__global__ void __launch_bounds__(kPoseTile) pnp_finish_kernel(const PnpParams p) {
    __shared__ int32_t kept[1][kPoseTile / 64];
    const int tid = threadIdx.x;
    const int j = blockIdx.x * kPoseTile + tid;
    const int m = min(p.m[0], p.n);
    const bool ok = p.flags[kFlagOk] != 0;
    float ps[7], R[9];
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        ps[e] = p.state[e];
    }
    if (ps[0] < 0.0f) {
        ps[0] = -ps[0], ps[1] = -ps[1], ps[2] = -ps[2], ps[3] = -ps[3];
    }
    pnp_rotation(ps, R);
    if (blockIdx.x == 0 && tid == 0) {
#pragma unroll
        for (int e = 0; e < 7; ++e) {
            p.pose[e] = ok ? ps[e] : (e == 0 ? 1.0f : 0.0f);
        }
        p.out_valid[0] = ok ? 1 : -1;
        p.best[0] = ok ? p.flags[kFlagWinner] : -1;
    }
    bool keep = false;
    if (ok && j < m) {
        const float4 q = p.points[j];
        float c[3];
        pnp_camera(R, ps, q.z, q.w, p.depth[j], c);
        keep = pnp_inlier(c, q.x, q.y, p.ry, p.tn2);
        if (!keep) {
            const int32_t i = p.list[j];
            if (i >= 0 && i < p.n) {
                p.status[i] = FTK_LARGE_RESIDUAL;
            }
        }
    }
    const bool flags[1] = {keep};
    pose_block_counts_add(kept, flags, p.n_inliers);
}

}  // namespace

hipError_t pnp_launch(const PnpPlan &plan, const PnpParams &p, hipStream_t stream) {
    PnpParams q = p;
    q.scan_per_thread = plan.scan_per_thread;
    q.select_per_thread = plan.select_per_thread;
    q.sample = plan.sample;
    hipLaunchKernelGGL(pnp_scan_kernel, dim3(1), dim3(kEpipolarScanBlock), 0, stream, q);
    if (plan.sampler == PnpSample::P3p) {
        hipLaunchKernelGGL(pnp_p3p_hypothesis_kernel, dim3(plan.hyp_blocks), dim3(kEpipolarHypBlock), 0, stream, q);
    } else {
        hipLaunchKernelGGL(pnp_hypothesis_kernel, dim3(plan.hyp_blocks), dim3(kEpipolarHypBlock), 0, stream, q);
    }
    hipLaunchKernelGGL(pnp_score_kernel, dim3(plan.score_tiles, plan.score_groups), dim3(kEpipolarScoreTile), 0, stream, q);
    hipLaunchKernelGGL(pnp_select_kernel, dim3(1), dim3(kEpipolarScanBlock), 0, stream, q);
    for (int32_t step = 0; step < plan.refine_iterations; ++step) {
        q.step = step;
        hipLaunchKernelGGL(pnp_sums_kernel, dim3(plan.tiles), dim3(kPoseTile), 0, stream, q);
        hipLaunchKernelGGL(pnp_step_kernel, dim3(1), dim3(kPoseSolveBlock), 0, stream, q);
    }
    hipLaunchKernelGGL(pnp_finish_kernel, dim3(plan.tiles), dim3(kPoseTile), 0, stream, q);
    return hipGetLastError();
}

}  // namespace ftk
