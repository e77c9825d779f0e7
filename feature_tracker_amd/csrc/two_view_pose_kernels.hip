// two_view_pose_kernels.hip — TwoViewPose on gfx950: the relative pose of two views and the landmarks of their inliers,
// everything on the device, five launches of fixed shape.
//
//  * pose_scan_kernel: the filters' scan (epipolar_device.h's ep_scan_participants: ONE workgroup lists the participants, status ==
//    FTK_TRACKED, in ascending index order) storing the CALIBRATED coordinates x = (u - cx) / fx of each view's own camera.
//  * pose_moment_kernel: the hot path.  A workgroup owns a tile of 256 participants; a thread forms its participant's epipolar row and the
//    45 distinct products of r r^T, and the tile reduces them in LDS by the STATED tree (p[j] += p[j + stride], stride 128 .. 1).  The
//    (entry, j) pairs of a step are dealt to all 256 threads, so a step costs ceil(45 stride / 256) adds per thread, not 45; the
//    operands of every add are the tree's, so the bits are.  No float atomics: a tile's 45 totals go to the workspace.
//  * pose_solve_kernel: ONE wave.  Lanes 0 .. 44 add the tile totals in ascending tile order; jacobi_eigen<9> finds the null vector,
//    jacobi_eigen<3> on E^T E the projection onto the essential matrices; the four candidates go to the workspace.  The matrices live
//    in LDS (run-time indices: no scratch); a rotation's row updates of A and of V run on lanes 0 .. N-1 and 16 .. 16+N-1, each the
//    restatement's expression on the restatement's operands.
//  * pose_count_kernel: per candidate the participants in front of both cameras, by ballot and popcount, ONE integer atomicAdd per
//    workgroup and candidate.
//  * pose_finish_kernel: a thread per point selects the winner, forms the pose (uniform arithmetic, every thread the same), triangulates
//    its point, tests its reprojection and rewrites its status; block 0 writes the pose.
// Every float operation below is stated in DESIGN.md 5.29 and restated in tests/two_view_pose_ref.c; the build has no contraction
// (-ffp-contract=off) and correctly rounded division and square root.
#include "epipolar_device.h"
#include "two_view_pose_plan.h"

namespace ftk {
namespace {

constexpr int kModelE = 0, kModelRa = 9, kModelRb = 18, kModelT = 27, kModelOk = 30;

__global__ void __launch_bounds__(kEpipolarScanBlock) pose_scan_kernel(const TwoViewPoseParams p) {
    __shared__ int32_t scan[kEpipolarScanBlock];
    ep_scan_participants(scan, p.status, p.n, p.scan_per_thread, p.m, [&](const int at, const int i) {
        const float2 r = reinterpret_cast<const float2 *>(p.ref_uv)[i];
        const float2 c = reinterpret_cast<const float2 *>(p.cur_uv)[i];
        p.points[at] = make_float4((r.x - p.cx1) / p.fx1, (r.y - p.cy1) / p.fy1, (c.x - p.cx2) / p.fx2, (c.y - p.cy2) / p.fy2);
    });
}

__global__ void __launch_bounds__(kPoseTile) pose_moment_kernel(const TwoViewPoseParams p) {
    __shared__ float tree[kPoseMoments][kPoseTile];
    const int m = min(p.m[0], p.n);
    const int base = blockIdx.x * kPoseTile;
    if (m < kEpipolarSample || base >= m) {
        return;  // the whole workgroup: the grid covers n, the solve kernel reads the tiles below M alone
    }
    const int tid = threadIdx.x;
    float r[9];
    bool use = base + tid < m;
    if (use) {
        const float4 q = p.points[base + tid];
        use = ep_finite(q.x) && ep_finite(q.y) && ep_finite(q.z) && ep_finite(q.w);
        r[0] = q.z * q.x, r[1] = q.z * q.y, r[2] = q.z, r[3] = q.w * q.x, r[4] = q.w * q.y, r[5] = q.w, r[6] = q.x, r[7] = q.y, r[8] = 1.0f;
    }
    {
        int e = 0;
#pragma unroll
        for (int a = 0; a < 9; ++a) {
#pragma unroll
            for (int b = a; b < 9; ++b, ++e) {
                tree[e][tid] = use ? r[a] * r[b] : 0.0f;
            }
        }
    }
    __syncthreads();
    for (int stride = kPoseTile / 2, shift = 7; stride >= 1; stride >>= 1, --shift) {
        const int jobs = kPoseMoments * stride;
        for (int job = tid; job < jobs; job += kPoseTile) {
            const int e = job >> shift, j = job & (stride - 1);
            tree[e][j] = tree[e][j] + tree[e][j + stride];
        }
        __syncthreads();
    }
    if (tid < kPoseMoments) {
        p.totals[(size_t)blockIdx.x * kPoseMoments + tid] = tree[tid][0];
    }
}

// Cyclic Jacobi on the symmetric N x N matrix a (LDS, full storage, row-major; its diagonal ends as the eigenvalues), eigenvectors
// accumulated in the columns of v (LDS).  Called by the whole workgroup of kPoseSolveBlock threads; a is complete and visible on entry,
// a and v are on return.  Pairs (p, q), p < q, in row-major order; kPoseJacobiSweeps sweeps, all of them.
template <int N>
__device__ __forceinline__ void jacobi_eigen(float *const a, float *const v, const int tid) {
    static_assert(16 + N <= kPoseSolveBlock, "the lanes of a rotation");
    for (int idx = tid; idx < N * N; idx += kPoseSolveBlock) {
        v[idx] = idx / N == idx % N ? 1.0f : 0.0f;
    }
    __syncthreads();
    for (int sweep = 0; sweep < kPoseJacobiSweeps; ++sweep) {
        for (int p = 0; p < N - 1; ++p) {
            for (int q = p + 1; q < N; ++q) {
                const float apq = a[p * N + q], app = a[p * N + p], aqq = a[q * N + q];
                __syncthreads();  // every lane has read the pair before any lane writes
                if (apq == 0.0f) {
                    continue;  // (wave-uniform, as every branch on the pair's three entries)
                }
                const float g = 100.0f * fabsf(apq);
                if (fabsf(app) + g == fabsf(app) && fabsf(aqq) + g == fabsf(aqq)) {  // negligible: set to zero, no rotation
                    if (tid == 0) {
                        a[p * N + q] = 0.0f;
                        a[q * N + p] = 0.0f;
                    }
                    __syncthreads();
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
                if (tid < N) {
                    const int r = tid;
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
                } else if (tid >= 16 && tid < 16 + N) {
                    const int r = tid - 16;
                    const float x = v[r * N + p], y = v[r * N + q];
                    v[r * N + p] = x - s * (y + x * tau);
                    v[r * N + q] = y + s * (x - y * tau);
                }
                __syncthreads();
            }
        }
    }
}

__global__ void __launch_bounds__(kPoseSolveBlock) pose_solve_kernel(const TwoViewPoseParams p) {
    __shared__ float a9[81], v9[81], a3[9], v3[9];
    const int tid = threadIdx.x;
    const int m = min(p.m[0], p.n);
    if (tid < 4) {
        p.n_front[tid] = 0;
    }
    if (tid == 0) {
        p.n_points[0] = 0;
    }
    if (m < kEpipolarSample) {
        if (tid < kPoseModelFloats) {
            p.model[tid] = 0.0f;
        }
        return;
    }
    // the 45 sums: tile totals in ascending tile order from +0
    if (tid < kPoseMoments) {
        const int tiles = (m + kPoseTile - 1) / kPoseTile;
        float acc = 0.0f;
        for (int t = 0; t < tiles; ++t) {
            acc = acc + p.totals[(size_t)t * kPoseMoments + tid];
        }
        int row = 0, rem = tid;
        while (rem >= 9 - row) {
            rem -= 9 - row;
            ++row;
        }
        const int col = row + rem;
        a9[row * 9 + col] = acc;
        a9[col * 9 + row] = acc;
    }
    __syncthreads();
    // the null vector: the eigenvector of the smallest eigenvalue, ties to the lowest column
    jacobi_eigen<9>(a9, v9, tid);
    int k = 0;
    for (int j = 1; j < 9; ++j) {
        if (a9[j * 9 + j] < a9[k * 9 + k]) {
            k = j;
        }
    }
    // the rank test: the second-smallest eigenvalue (ties to the lowest column) must exceed 2^-20 of the largest
    int k2 = k == 0 ? 1 : 0;
    float lmax = a9[0];
    for (int j = 1; j < 9; ++j) {
        if (j != k && a9[j * 9 + j] < a9[k2 * 9 + k2]) {
            k2 = j;
        }
        if (a9[j * 9 + j] > lmax) {
            lmax = a9[j * 9 + j];
        }
    }
    const bool rank_ok = a9[k2 * 9 + k2] > kPoseRankFloor * lmax;
    float E[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        E[i] = v9[i * 9 + k];
    }
    // the essential projection: E^T E = V diag(sigma^2) V^T
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                a3[i * 3 + j] = (E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j];
            }
        }
    }
    __syncthreads();
    jacobi_eigen<3>(a3, v3, tid);
    const float l0 = a3[0], l1 = a3[4], l2 = a3[8];
    int i1 = 0;
    if (l1 > l0) {
        i1 = 1;
    }
    if (l2 > (i1 == 0 ? l0 : l1)) {
        i1 = 2;
    }
    const int ia = i1 == 0 ? 1 : 0, ib = i1 == 2 ? 1 : 2;  // the other two, ascending
    const int i2 = a3[ib * 4] > a3[ia * 4] ? ib : ia;
    const float s1 = sqrtf(a3[i1 * 4]), s2 = sqrtf(a3[i2 * 4]);
    float v1[3], v2[3], v3v[3], u1[3], u2[3], u3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v1[i] = v3[i * 3 + i1];
        v2[i] = v3[i * 3 + i2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u1[i] = ((E[i * 3] * v1[0] + E[i * 3 + 1] * v1[1]) + E[i * 3 + 2] * v1[2]) / s1;
        u2[i] = ((E[i * 3] * v2[0] + E[i * 3 + 1] * v2[1]) + E[i * 3 + 2] * v2[2]) / s2;
    }
    v3v[0] = v1[1] * v2[2] - v1[2] * v2[1], v3v[1] = v1[2] * v2[0] - v1[0] * v2[2], v3v[2] = v1[0] * v2[1] - v1[1] * v2[0];
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1], u3[1] = u1[2] * u2[0] - u1[0] * u2[2], u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    if (tid == 0) {
        bool ok = rank_ok;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float eh = u1[i] * v1[j] + u2[i] * v2[j];
                const float ra = (u2[i] * v1[j] - u1[i] * v2[j]) + u3[i] * v3v[j];
                const float rb = (u1[i] * v2[j] - u2[i] * v1[j]) + u3[i] * v3v[j];
                p.model[kModelE + i * 3 + j] = eh;
                p.model[kModelRa + i * 3 + j] = ra;
                p.model[kModelRb + i * 3 + j] = rb;
                ok = ok && ep_finite(eh) && ep_finite(ra) && ep_finite(rb);
            }
            p.model[kModelT + i] = u3[i];
        }
        ok = ok && ep_finite(u3[0]) && ep_finite(u3[1]) && ep_finite(u3[2]);
        p.model[kModelOk] = ok ? 1.0f : 0.0f;
        p.model[kModelOk + 1] = 0.0f;
    }
}

// a = R (x, y, 1)
__device__ __forceinline__ void pose_rotate(const float (&R)[9], const float x, const float y, float (&a)[3]) {
    a[0] = (R[0] * x + R[1] * y) + R[2];
    a[1] = (R[3] * x + R[4] * y) + R[5];
    a[2] = (R[6] * x + R[7] * y) + R[8];
}

// The two-ray depths of z2 (x2, y2, 1) = z1 R (x1, y1, 1) + t by the 2 x 2 normal equations of the midpoint; true: both finite and > 0.
__device__ __forceinline__ bool pose_in_front(const float (&R)[9], const float (&t)[3], const float4 q, float &z1, float &z2) {
    z1 = 0.0f;
    z2 = 0.0f;
    if (!(ep_finite(q.x) && ep_finite(q.y) && ep_finite(q.z) && ep_finite(q.w))) {
        return false;
    }
    float a[3];
    pose_rotate(R, q.x, q.y, a);
    const float b[3] = {q.z, q.w, 1.0f};
    float aa, bb, ab;
    return ep_two_ray_depths(a, b, t, z1, z2, aa, bb, ab);
}

// Candidate c = 2 * (R is Rb) + (t is -u3), from the model block.
__device__ __forceinline__ void pose_candidate(const float *const model, const int c, float (&R)[9], float (&t)[3]) {
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        R[e] = c < 2 ? model[kModelRa + e] : model[kModelRb + e];
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const float u = model[kModelT + e];
        t[e] = (c & 1) ? -u : u;
    }
}

__global__ void __launch_bounds__(kPoseTile) pose_count_kernel(const TwoViewPoseParams p) {
    __shared__ int32_t counts[4][kPoseTile / 64];
    const int m = min(p.m[0], p.n);
    const int base = blockIdx.x * kPoseTile;
    if (m < kEpipolarSample || base >= m || p.model[kModelOk] == 0.0f) {
        return;  // the whole workgroup
    }
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool active = base + tid < m;
    const float4 q = active ? p.points[base + tid] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float R[9], t[3], z1, z2;
        pose_candidate(p.model, c, R, t);
        const bool in = active && pose_in_front(R, t, q, z1, z2);
        const int32_t count = (int32_t)__popcll(__ballot(in));
        if (lane == 0) {
            counts[c][wave] = count;
        }
    }
    __syncthreads();
    if (tid < 4) {
        int32_t sum = 0;
#pragma unroll
        for (int w = 0; w < kPoseTile / 64; ++w) {
            sum += counts[tid][w];
        }
        if (sum > 0) {
            atomicAdd(&p.n_front[tid], sum);
        }
    }
}

__global__ void __launch_bounds__(kPoseTile) pose_finish_kernel(const TwoViewPoseParams p) {
    __shared__ int32_t kept[kPoseTile / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = blockIdx.x * kPoseTile + tid;
    const int m = min(p.m[0], p.n);
    bool ok = m >= kEpipolarSample && p.model[kModelOk] != 0.0f;
    // the winner: the greatest count, the lowest candidate among equals
    int win = 0;
    int32_t best = 0;
    if (ok) {
        best = p.n_front[0];
#pragma unroll
        for (int c = 1; c < 4; ++c) {
            const int32_t count = p.n_front[c];
            if (count > best) {
                best = count;
                win = c;
            }
        }
        ok = best > 0;
    }
    float R[9] = {}, t[3] = {}, ps[7] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float sc = 0.0f;
    if (ok) {
        // the pose in DirectMethod's convention: R_rc = R^T, p_rc = -R^T t scaled to the baseline
        pose_candidate(p.model, win, R, t);
        const float nt = sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
        sc = p.baseline / nt;
        const float ts0 = t[0] * sc, ts1 = t[1] * sc, ts2 = t[2] * sc;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            ps[4 + j] = -((R[j] * ts0 + R[3 + j] * ts1) + R[6 + j] * ts2);
        }
        // Shepperd on M = R^T: M(i, j) = R[j * 3 + i]
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
#pragma unroll
        for (int e = 0; e < 7; ++e) {
            ok = ok && ep_finite(ps[e]);
        }
    }
    if (blockIdx.x == 0) {
        if (tid < 9) {
            p.E[tid] = ok ? p.model[kModelE + tid] : 0.0f;
        }
        if (tid == 0) {
#pragma unroll
            for (int e = 0; e < 7; ++e) {  // (ps is indexed at compile time alone: it stays in registers)
                p.pose[e] = ok ? ps[e] : (e == 0 ? 1.0f : 0.0f);
            }
            p.valid[0] = ok ? 1 : -1;
        }
    }
    // this thread's point: the landmark and the status
    bool keep = false;
    if (i < p.n) {
        float X = 0.0f, Y = 0.0f, Z = 0.0f;
        if (ok && p.status[i] == FTK_TRACKED) {
            const float2 r = reinterpret_cast<const float2 *>(p.ref_uv)[i];
            const float2 c = reinterpret_cast<const float2 *>(p.cur_uv)[i];
            const float4 q = make_float4((r.x - p.cx1) / p.fx1, (r.y - p.cy1) / p.fy1, (c.x - p.cx2) / p.fx2, (c.y - p.cy2) / p.fy2);
            float z1, z2;
            keep = pose_in_front(R, t, q, z1, z2);
            if (keep) {
                float a[3];
                pose_rotate(R, q.x, q.y, a);
                const float cX = z1 * a[0] + t[0], cY = z1 * a[1] + t[1], cZ = z1 * a[2] + t[2];
                const float ex = p.fx2 * (cX - q.z * cZ), ey = p.fy2 * (cY - q.w * cZ);
                const float lhs = ex * ex + ey * ey, rhs = p.t2 * (cZ * cZ);
                keep = ep_finite(lhs) && ep_finite(rhs) && lhs <= rhs;
            }
            if (keep) {
                const float zs = z1 * sc;
                X = zs * q.x, Y = zs * q.y, Z = zs;
            } else {
                p.status[i] = FTK_LARGE_RESIDUAL;
            }
        }
        p.landmarks[3 * (size_t)i] = X;
        p.landmarks[3 * (size_t)i + 1] = Y;
        p.landmarks[3 * (size_t)i + 2] = Z;
    }
    const int32_t count = (int32_t)__popcll(__ballot(keep));
    if (lane == 0) {
        kept[wave] = count;
    }
    __syncthreads();
    if (tid == 0) {
        int32_t sum = 0;
#pragma unroll
        for (int w = 0; w < kPoseTile / 64; ++w) {
            sum += kept[w];
        }
        if (sum > 0) {
            atomicAdd(&p.n_points[0], sum);
        }
    }
}

}  // namespace

hipError_t two_view_pose_launch(const TwoViewPosePlan &plan, const TwoViewPoseParams &p, hipStream_t stream) {
    TwoViewPoseParams q = p;
    q.scan_per_thread = plan.scan_per_thread;
    hipLaunchKernelGGL(pose_scan_kernel, dim3(1), dim3(kEpipolarScanBlock), 0, stream, q);
    hipLaunchKernelGGL(pose_moment_kernel, dim3(plan.tiles), dim3(kPoseTile), 0, stream, q);
    hipLaunchKernelGGL(pose_solve_kernel, dim3(1), dim3(kPoseSolveBlock), 0, stream, q);
    hipLaunchKernelGGL(pose_count_kernel, dim3(plan.tiles), dim3(kPoseTile), 0, stream, q);
    hipLaunchKernelGGL(pose_finish_kernel, dim3(plan.tiles), dim3(kPoseTile), 0, stream, q);
    return hipGetLastError();
}

}  // namespace ftk
