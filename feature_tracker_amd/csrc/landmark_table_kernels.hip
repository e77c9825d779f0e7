// landmark_table_kernels.hip — the landmark table beside a track table on gfx950: which slot's landmark belongs to
// which track, and a landmark for a track born after the first pair, by two-ray triangulation from two views whose poses are known.
// Two kernels, one thread per slot, workgroups of kLandmarkBlock = 256, every launch over all n slots:
//
//  * landmark_begin_kernel, before the frame's pose is known: a slot whose id is not its owner's changed hands (owner <- id, the landmark
//    zeroed, no anchor); pnp_status is TRACKED for a live slot that holds a landmark, anchor_status for a live slot that has an anchor,
//    FTK_NOT_TRACKED otherwise; block 0 zeroes the four counters that the end kernel adds to.
//  * landmark_end_kernel, after it: with an invalid pose `lost` grows and no slot changes; otherwise the pose is kept, a PnP outlier loses
//    its landmark, a live slot without landmark and anchor is anchored at this frame, and a slot anchored earlier is triangulated from its
//    anchor and this frame (it waits below the parallax floor; a failure anchors it again).  The counts are ballots and popcounts, ONE
//    integer atomicAdd per workgroup and counter: every output is a pure function of the inputs.
// Every float operation below is stated in DESIGN.md 5.31 and restated in tests/landmark_table_ref.c; the build has no contraction
// (-ffp-contract=off) and correctly rounded division.  The inlier rule, the rotation of a quaternion and the camera coordinates
// (pnp_inlier, pnp_rotation, pnp_camera), the rays and their depths (pose_ray, ep_two_ray_depths) and the end kernel's four counts
// (pose_block_counts_add) are pose_device.h's, shared with PnpRansac and TwoViewPose.
#include "pose_device.h"
#include "landmark_table_plan.h"

namespace ftk {
namespace {

constexpr int kWaits = 0, kFails = 1, kKept = 2;

// The landmark of a slot seen at the pixel (ua, va) from the pose pa and at (uc, vc) from the pose pc (rotation Rc), in the world frame.
__device__ __forceinline__ int landmark_triangulate(const LandmarkParams &p, const float (&pa)[7], const float ua, const float va, const float (&pc)[7],
                                                    const float (&Rc)[9], const float uc, const float vc, float (&X)[3]) {
    bool finite = ep_finite(ua) && ep_finite(va) && ep_finite(uc) && ep_finite(vc);
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        finite = finite && ep_finite(pa[e]) && ep_finite(pc[e]);
    }
    if (!finite) {
        return kFails;
    }
    const float xa = (ua - p.cx) / p.fx, ya = (va - p.cy) / p.fy;
    const float xc = (uc - p.cx) / p.fx, yc = (vc - p.cy) / p.fy;
    float Ra[9];
    pnp_rotation(pa, Ra);
    float a[3], b[3];
    pose_ray(Ra, xa, ya, a);
    pose_ray(Rc, xc, yc, b);
    const float t[3] = {pa[4] - pc[4], pa[5] - pc[5], pa[6] - pc[6]};
    float z1, z2, aa, bb, ab;
    const bool front = ep_two_ray_depths(a, b, t, z1, z2, aa, bb, ab);
    if (ab * ab > p.c2 * (aa * bb)) {
        return kWaits;  // the rays meet below the parallax floor
    }
    if (!front) {
        return kFails;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        X[k] = ((pa[4 + k] + z1 * a[k]) + (pc[4 + k] + z2 * b[k])) * 0.5f;
    }
    if (!(ep_finite(X[0]) && ep_finite(X[1]) && ep_finite(X[2])) || (X[0] == 0.0f && X[1] == 0.0f && X[2] == 0.0f)) {
        return kFails;
    }
    float ca[3], cc[3];
    pnp_camera(Ra, pa, X[0], X[1], X[2], ca);
    pnp_camera(Rc, pc, X[0], X[1], X[2], cc);
    return pnp_inlier(ca, xa, ya, p.ry, p.tn2) && pnp_inlier(cc, xc, yc, p.ry, p.tn2) ? kKept : kFails;
}

__global__ void __launch_bounds__(kLandmarkBlock) landmark_begin_kernel(const LandmarkParams p) {
    const int s = blockIdx.x * kLandmarkBlock + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // (nothing adds to them in this launch)
        p.counters[kLandmarkNew] = 0;
        p.counters[kLandmarkAnchored] = 0;
        p.counters[kLandmarkCount] = 0;
        p.counters[kLandmarkDropped] = 0;
    }
    if (s >= p.n) {
        return;  // (no barrier and no ballot below)
    }
    const int64_t id = p.ids[s];
    bool has, anchored;
    if (id != p.owner[s]) {  // the slot changed hands
        p.owner[s] = id;
        p.landmarks[3 * (size_t)s] = 0.0f, p.landmarks[3 * (size_t)s + 1] = 0.0f, p.landmarks[3 * (size_t)s + 2] = 0.0f;
        p.anchor_frame[s] = -1;
        has = false, anchored = false;
    } else {
        const float X = p.landmarks[3 * (size_t)s], Y = p.landmarks[3 * (size_t)s + 1], Z = p.landmarks[3 * (size_t)s + 2];
        has = !(X == 0.0f && Y == 0.0f && Z == 0.0f);
        anchored = p.anchor_frame[s] >= 0;
    }
    p.pnp_status[s] = id >= 0 && has ? FTK_TRACKED : FTK_NOT_TRACKED;
    p.anchor_status[s] = id >= 0 && anchored ? FTK_TRACKED : FTK_NOT_TRACKED;
}

__global__ void __launch_bounds__(kLandmarkBlock) landmark_end_kernel(const LandmarkParams p) {
    constexpr int kWaves = kLandmarkBlock / 64;
    __shared__ int32_t counts[4][kWaves];
    const int tid = threadIdx.x;
    const int s = blockIdx.x * kLandmarkBlock + tid;
    const bool ok = p.valid_in[0] == 1 && (p.model_in == nullptr || p.model_in[0] == 0);
    float pc[7];
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        pc[e] = p.pose_in[e];
    }
    if (blockIdx.x == 0 && tid == 0) {
        p.counters[kLandmarkValid] = ok ? 1 : -1;
        p.counters[kLandmarkLost] = ok ? 0 : p.counters[kLandmarkLost] + 1;
        if (ok) {
#pragma unroll
            for (int e = 0; e < 7; ++e) {
                p.pose[e] = pc[e];
            }
        }
    }
    const bool live = s < p.n && p.ids[s] >= 0;
    bool anchored = false, holds = false, is_new = false, dropped = false;
    if (live) {
        const float X0 = p.landmarks[3 * (size_t)s], Y0 = p.landmarks[3 * (size_t)s + 1], Z0 = p.landmarks[3 * (size_t)s + 2];
        holds = !(X0 == 0.0f && Y0 == 0.0f && Z0 == 0.0f);
        const int32_t frame_in = p.anchor_frame[s];
        anchored = frame_in >= 0;
        if (ok) {
            const bool steady = p.mode == kLandmarkSteady;
            const float2 uv = reinterpret_cast<const float2 *>(p.points)[s];
            bool has_anchor = anchored;
            if (steady && p.status_in[s] == FTK_LARGE_RESIDUAL) {  // rule a: a PnP outlier loses its landmark and its anchor
                p.landmarks[3 * (size_t)s] = 0.0f, p.landmarks[3 * (size_t)s + 1] = 0.0f, p.landmarks[3 * (size_t)s + 2] = 0.0f;
                holds = false, has_anchor = false, dropped = true;
            }
            bool anchor_now = steady && !holds && !has_anchor;  // rule b
            if (!holds && has_anchor) {                          // rule c: an anchor of an earlier call
                float pa[7], Rc[9], X[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int e = 0; e < 7; ++e) {
                    pa[e] = p.anchor_pose[7 * (size_t)s + e];
                }
                pnp_rotation(pc, Rc);
                const float2 at = reinterpret_cast<const float2 *>(p.anchor_uv)[s];
                const int outcome = landmark_triangulate(p, pa, at.x, at.y, pc, Rc, uv.x, uv.y, X);
                if (outcome == kKept) {
                    p.landmarks[3 * (size_t)s] = X[0], p.landmarks[3 * (size_t)s + 1] = X[1], p.landmarks[3 * (size_t)s + 2] = X[2];
                    holds = true, is_new = true;
                } else if (outcome == kFails && steady) {
                    anchor_now = true;
                }
            }
            if (anchor_now) {
                reinterpret_cast<float2 *>(p.anchor_uv)[s] = uv;
#pragma unroll
                for (int e = 0; e < 7; ++e) {
                    p.anchor_pose[7 * (size_t)s + e] = pc[e];
                }
                p.anchor_frame[s] = p.frame;  // (a slot that rule a dropped always arrives here: its anchor_frame = -1 is never seen)
            }
        }
    }
    const bool flags[4] = {is_new, anchored, holds, dropped};
    pose_block_counts_add(counts, flags, &p.counters[kLandmarkNew]);  // kLandmarkNew, kLandmarkAnchored, kLandmarkCount, kLandmarkDropped are consecutive
}

}  // namespace

static_assert(kLandmarkAnchored == kLandmarkNew + 1 && kLandmarkCount == kLandmarkNew + 2 && kLandmarkDropped == kLandmarkNew + 3, "the end kernel's counter order");

hipError_t landmark_begin_launch(const LandmarkPlan &plan, const LandmarkParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(landmark_begin_kernel, dim3(plan.blocks), dim3(kLandmarkBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t landmark_end_launch(const LandmarkPlan &plan, const LandmarkParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(landmark_end_kernel, dim3(plan.blocks), dim3(kLandmarkBlock), 0, stream, p);
    return hipGetLastError();
}

}  // namespace ftk
