// two_view_pose_kernels.hip — TwoViewPose on gfx950: the relative pose of two views and the landmarks of their inliers,
// everything on the device, five launches of fixed shape.
//
//  * pose_scan_kernel: the filters' scan (epipolar_device.h's ep_scan_participants: ONE workgroup lists the participants, status ==
//    FTK_TRACKED, in ascending index order) storing the CALIBRATED coordinates x = (u - cx) / fx of each view's own camera.
//  * pose_moment_kernel: the hot path.  A workgroup owns a tile of 256 participants; a thread forms its participant's epipolar row and the
//    45 distinct products of r r^T, and the tile reduces them in LDS by the STATED tree (pose_device.h's pose_tree_sum: p[j] += p[j +
//    stride], stride 128 .. 1).  The (entry, j) pairs of a step are dealt to all 256 threads, so a step costs ceil(45 stride / 256) adds
//    per thread, not 45; the operands of every add are the tree's, so the bits are.  No float atomics: a tile's 45 totals go to the
//    workspace.
//  * pose_solve_kernel: ONE wave.  Lanes 0 .. 44 add the tile totals in ascending tile order (pose_tile_total); pose_device.h's
//    jacobi_eigen<9, Jacobi::Wave> finds the null vector, jacobi_eigen<3, Jacobi::Wave> on E^T E the projection onto the essential
//    matrices; the four candidates go to the workspace.  The matrices live in LDS (run-time indices: no scratch); a rotation's row
//    updates of A and of V run on lanes 0 .. N-1 and 16 .. 16+N-1, each the restatement's expression on the restatement's operands.
//  * pose_count_kernel: per candidate the participants in front of both cameras (pose_ray, ep_two_ray_depths), counted by
//    pose_block_counts_add: ballot and popcount, ONE integer atomicAdd per workgroup and candidate.
//  * pose_finish_kernel: a thread per point selects the winner, forms the pose (uniform arithmetic, every thread the same; the quaternion
//    is pose_quaternion_of_transpose), triangulates its point, tests its reprojection and rewrites its status; block 0 writes the pose.
// Every float operation below is stated in DESIGN.md 5.29 and restated in tests/two_view_pose_ref.c; the build has no contraction
// (-ffp-contract=off) and correctly rounded division and square root.
#include "pose_device.h"

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
    pose_tree_sum(tree, tid);
    if (tid < kPoseMoments) {
        p.totals[(size_t)blockIdx.x * kPoseMoments + tid] = tree[tid][0];
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
        const float acc = pose_tile_total(p.totals, (m + kPoseTile - 1) / kPoseTile, kPoseMoments, tid);
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
    jacobi_eigen<9, Jacobi::Wave>(a9, v9, tid);
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
    jacobi_eigen<3, Jacobi::Wave>(a3, v3, tid);
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

// The two-ray depths of z2 (x2, y2, 1) = z1 R (x1, y1, 1) + t by the 2 x 2 normal equations of the midpoint; true: both finite and > 0.
__device__ __forceinline__ bool pose_in_front(const float (&R)[9], const float (&t)[3], const float4 q, float &z1, float &z2) {
    z1 = 0.0f;
    z2 = 0.0f;
    if (!(ep_finite(q.x) && ep_finite(q.y) && ep_finite(q.z) && ep_finite(q.w))) {
        return false;
    }
    float a[3];
    pose_ray(R, q.x, q.y, a);
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
    const int tid = threadIdx.x;
    const bool active = base + tid < m;
    const float4 q = active ? p.points[base + tid] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool in[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float R[9], t[3], z1, z2;
        pose_candidate(p.model, c, R, t);
        in[c] = active && pose_in_front(R, t, q, z1, z2);
    }
    pose_block_counts_add(counts, in, p.n_front);
}

__global__ void __launch_bounds__(kPoseTile) pose_finish_kernel(const TwoViewPoseParams p) {
    __shared__ int32_t kept[1][kPoseTile / 64];
    const int tid = threadIdx.x;
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
        pose_quaternion_of_transpose(R, ps);
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
                pose_ray(R, q.x, q.y, a);
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
    const bool flags[1] = {keep};
    pose_block_counts_add(kept, flags, p.n_points);
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
