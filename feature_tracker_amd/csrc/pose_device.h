// pose_device.h — the pose geometry and the reductions that the kernels after the RANSAC stages share.  Each is stated here once:
//
//  * pnp_inlier, pnp_rotation, pnp_camera: pnp_score / pnp_sums / pnp_step / pnp_finish_kernel, landmark_end_kernel.
//  * pose_ray, ep_two_ray_depths: pose_count / pose_finish_kernel, landmark_end_kernel.
//  * pose_quaternion_of_transpose (Shepperd): pose_finish_kernel, pnp_select_kernel.
//  * jacobi_eigen<N, Jacobi::Wave>: pose_solve_kernel; jacobi_eigen<3, Jacobi::Thread>: pnp_select_kernel.
//  * pose_tree_sum<K>: pose_moment_kernel (K = 45), pnp_sums_kernel (K = 27); pose_tile_total: pose_solve_kernel, pnp_step_kernel.
//  * pose_block_counts, pose_block_counts_add: pose_count / pose_finish_kernel, pnp_sums / pnp_finish_kernel, landmark_end_kernel.
//
// Every float operation is stated in DESIGN.md 5.29, 5.30 and 5.31 and restated in tests/two_view_pose_ref.c, tests/pnp_ref.c and
// tests/landmark_table_ref.c; the build has no contraction (-ffp-contract=off) and correctly rounded division and square root.
#pragma once

#include "epipolar_device.h"
#include "two_view_pose_plan.h"

namespace ftk {

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

// The ray a = R (x, y, 1).
__device__ __forceinline__ void pose_ray(const float (&R)[9], const float x, const float y, float (&a)[3]) {
    a[0] = (R[0] * x + R[1] * y) + R[2];
    a[1] = (R[3] * x + R[4] * y) + R[5];
    a[2] = (R[6] * x + R[7] * y) + R[8];
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

// Shepperd's unit quaternion (w >= 0) of M = R^T, M(i, j) = R[j * 3 + i], into ps[0 .. 3]: DirectMethod's convention R_rc = R^T.
__device__ __forceinline__ void pose_quaternion_of_transpose(const float (&R)[9], float (&ps)[7]) {
    const float m00 = R[0], m01 = R[3], m02 = R[6], m10 = R[1], m11 = R[4], m12 = R[7], m20 = R[2], m21 = R[5], m22 = R[8];
    const float tr = (m00 + m11) + m22;
    float qw, qx, qy, qz;
    if (tr > 0.0f) {
        const float s = sqrtf(tr + 1.0f) * 2.0f;
        qw = 0.25f * s, qx = (m21 - m12) / s, qy = (m02 - m20) / s, qz = (m10 - m01) / s;
    } else if (m00 > m11 && m00 > m22) {
        const float s = sqrtf(((1.0f + m00) - m11) - m22) * 2.0f;
        qw = (m21 - m12) / s, qx = 0.25f * s, qy = (m01 + m10) / s, qz = (m02 + m20) / s;
    } else if (m11 > m22) {
        const float s = sqrtf(((1.0f + m11) - m00) - m22) * 2.0f;
        qw = (m02 - m20) / s, qx = (m01 + m10) / s, qy = 0.25f * s, qz = (m12 + m21) / s;
    } else {
        const float s = sqrtf(((1.0f + m22) - m00) - m11) * 2.0f;
        qw = (m10 - m01) / s, qx = (m02 + m20) / s, qy = (m12 + m21) / s, qz = 0.25f * s;
    }
    if (qw < 0.0f) {
        qw = -qw, qx = -qx, qy = -qy, qz = -qz;
    }
    const float qn = sqrtf(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    ps[0] = qw / qn, ps[1] = qx / qn, ps[2] = qy / qn, ps[3] = qz / qn;
}

// Cyclic Jacobi on the symmetric N x N matrix a (LDS, full storage, row-major, run-time indices: no scratch; its diagonal ends as the
// eigenvalues), eigenvectors accumulated in the columns of v (LDS).  Pairs (p, q), p < q, in row-major order; kPoseJacobiSweeps sweeps,
// all of them.  Who runs it is chosen at compile time:
//  * Jacobi::Wave: the whole workgroup of kPoseSolveBlock threads calls it.  a is complete and visible on entry, a and v are on return.
//    A rotation's row r of a is lane r's, its row r of v lane 16 + r's; every lane computes the (wave-uniform) decision and scalars.
//  * Jacobi::Thread: ONE thread calls it with tid = 0 and loops over the rows; no barrier.
enum class Jacobi { Wave, Thread };

template <int N, Jacobi By>
__device__ __forceinline__ void jacobi_eigen(float *const a, float *const v, const int tid) {
    constexpr bool kWave = By == Jacobi::Wave;
    static_assert(16 + N <= kPoseSolveBlock, "the lanes of a rotation");
    const auto barrier = [] {
        if constexpr (kWave) {
            __syncthreads();
        }
    };
    for (int idx = tid; idx < N * N; idx += kWave ? kPoseSolveBlock : 1) {
        v[idx] = idx / N == idx % N ? 1.0f : 0.0f;
    }
    barrier();
    for (int sweep = 0; sweep < kPoseJacobiSweeps; ++sweep) {
        for (int p = 0; p < N - 1; ++p) {
            for (int q = p + 1; q < N; ++q) {
                const float apq = a[p * N + q], app = a[p * N + p], aqq = a[q * N + q];
                barrier();  // every lane has read the pair before any lane writes
                if (apq == 0.0f) {
                    continue;  // (wave-uniform, as every branch on the pair's three entries)
                }
                const float g = 100.0f * fabsf(apq);
                if (fabsf(app) + g == fabsf(app) && fabsf(aqq) + g == fabsf(aqq)) {  // negligible: set to zero, no rotation
                    if (tid == 0) {
                        a[p * N + q] = 0.0f;
                        a[q * N + p] = 0.0f;
                    }
                    barrier();
                    continue;
                }
                const float h = aqq - app;
                float t;
                if (fabsf(h) + g == fabsf(h)) {
                    t = apq / h;
                } else {
                    const float theta = h / (2.0f * apq);
                    t = 1.0f / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
                    if (theta < 0.0f) {
                        t = -t;
                    }
                }
                const float c = 1.0f / sqrtf(t * t + 1.0f);
                const float s = t * c;
                const float tau = s / (1.0f + c);
                const float hh = t * apq;
                const auto row_of_a = [&](const int r) {  // (the rows write disjoint entries: their order is free)
                    if (r == p) {
                        a[p * N + p] = app - hh;
                        a[q * N + q] = aqq + hh;
                        a[p * N + q] = 0.0f;
                        a[q * N + p] = 0.0f;
                    } else if (r != q) {
                        const float x = a[r * N + p], y = a[r * N + q];
                        const float xn = x - s * (y + x * tau), yn = y + s * (x - y * tau);
                        a[r * N + p] = xn;
                        a[p * N + r] = xn;
                        a[r * N + q] = yn;
                        a[q * N + r] = yn;
                    }
                };
                const auto row_of_v = [&](const int r) {
                    const float x = v[r * N + p], y = v[r * N + q];
                    v[r * N + p] = x - s * (y + x * tau);
                    v[r * N + q] = y + s * (x - y * tau);
                };
                if constexpr (kWave) {
                    if (tid < N) {
                        row_of_a(tid);
                    } else if (tid >= 16 && tid < 16 + N) {
                        row_of_v(tid - 16);
                    }
                    __syncthreads();
                } else {
                    for (int r = 0; r < N; ++r) {
                        row_of_a(r);
                        row_of_v(r);
                    }
                }
            }
        }
    }
}

// The STATED summation tree of a tile of kPoseTile participants, K sums at once: tree[e][j] += tree[e][j + stride], stride 128 .. 1; a
// step's (entry, j) pairs are dealt to all kPoseTile threads.  tree is complete and visible on entry (the caller's barrier); tree[e][0]
// is entry e's total, visible to every thread, on return.
template <int K>
__device__ __forceinline__ void pose_tree_sum(float (&tree)[K][kPoseTile], const int tid) {
    for (int stride = kPoseTile / 2, shift = 7; stride >= 1; stride >>= 1, --shift) {
        const int jobs = K * stride;
        for (int job = tid; job < jobs; job += kPoseTile) {
            const int e = job >> shift, j = job & (stride - 1);
            tree[e][j] = tree[e][j] + tree[e][j + stride];
        }
        __syncthreads();
    }
}

// Entry e of the K sums over all tiles: the tile totals in ascending tile order from +0.
__device__ __forceinline__ float pose_tile_total(const float *const totals, const int tiles, const int K, const int e) {
    float acc = 0.0f;
    for (int t = 0; t < tiles; ++t) {
        acc = acc + totals[(size_t)t * K + e];
    }
    return acc;
}

// The workgroup's number of threads whose flags[c] is set, for C flags at once: ballot and popcount, one int per wave and flag in LDS
// (counts), a barrier, then thread c hands flag c's sum over the waves to emit(c, sum).  Called by every thread of the workgroup.
template <int C, int WAVES, class Emit>
__device__ __forceinline__ void pose_block_counts(int32_t (&counts)[C][WAVES], const bool (&flags)[C], Emit emit) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int32_t count = (int32_t)__popcll(__ballot(flags[c]));
        if (lane == 0) {
            counts[c][wave] = count;
        }
    }
    __syncthreads();
    if (tid < C) {
        int32_t sum = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            sum += counts[tid][w];
        }
        emit(tid, sum);
    }
}

// ... added to total[c]: ONE integer atomicAdd per workgroup and flag, none for a sum of zero.
template <int C, int WAVES>
__device__ __forceinline__ void pose_block_counts_add(int32_t (&counts)[C][WAVES], const bool (&flags)[C], int32_t *const total) {
    pose_block_counts(counts, flags, [&](const int c, const int32_t sum) {
        if (sum > 0) {
            atomicAdd(&total[c], sum);
        }
    });
}

}  // namespace ftk
