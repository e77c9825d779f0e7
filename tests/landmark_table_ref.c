/* landmark_table_ref.c — the scalar CPU restatement of the landmark table's two kernels: which slot's landmark belongs to
 * which track, and the two-ray triangulation of a track born after the first pair.
 *
 * TEST INFRASTRUCTURE ONLY.  Every float operation of the contract in the order DESIGN.md 5.31 states it, float32, compiled without
 * contraction (tests/ref_build.py's STRICT flags); `/` is correctly rounded.  The device (csrc/landmark_table_kernels.hip) is held to this
 * file bit for bit by tests/test_track_odometry_gpu.py; tests/test_track_odometry_cpu.py pins this file to an independent float64
 * restatement (tests/landmark_table_ref64.py) and to ground truth.  `variant` 0 is the contract; the others are the mutants that the CPU
 * tests must catch.  `outcome` (may be NULL) records what rule c did with each slot; it reads values the contract computes and changes
 * none of them.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { NOT_TRACKED = 0, TRACKED = 1, LARGE_RESIDUAL = 2 };
enum { C_VALID = 0, C_NEW = 1, C_ANCHORED = 2, C_LANDMARKS = 3, C_DROPPED = 4, C_LOST = 5 };
enum { STEADY = 0, BOOTSTRAP = 1 };
enum { CONTRACT = 0, OWNER_CHANGE_KEEPS_LANDMARK = 1, PARALLAX_TEST_OMITTED = 2, T_WITH_THE_OTHER_SIGN = 3, NO_REANCHOR = 4, ONE_RAY = 5,
       RULE_C_OFF = 6 /* no mutant: the contrast of the sequence test, a table that triangulates in the bootstrap alone */ };
enum { O_NONE = -1, O_WAITS = 0, O_FAILS = 1, O_KEPT = 2 };

static int finite32(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x7F800000u) != 0x7F800000u;
}

/* PnpRansac's inlier rule (tests/pnp_ref.c: inlier). */
static int inlier(float c0, float c1, float c2, float x, float y, float ry, float tn2) {
    const float ex = c0 - x * c2;
    const float ey = (c1 - y * c2) * ry;
    const float lhs = ex * ex + ey * ey, rhs = tn2 * (c2 * c2);
    return c2 > 0.0f && finite32(lhs) && finite32(rhs) && lhs <= rhs;
}

/* R_rc of a unit quaternion (w, x, y, z), row-major (tests/pnp_ref.c: rotation_of). */
static void rotation_of(const float *q, float *R) {
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0f - 2.0f * (y * y + z * z), R[1] = 2.0f * (x * y - w * z), R[2] = 2.0f * (x * z + w * y);
    R[3] = 2.0f * (x * y + w * z), R[4] = 1.0f - 2.0f * (x * x + z * z), R[5] = 2.0f * (y * z - w * x);
    R[6] = 2.0f * (x * z - w * y), R[7] = 2.0f * (y * z + w * x), R[8] = 1.0f - 2.0f * (x * x + y * y);
}

/* c = R_rc^T (X - p_rc) (tests/pnp_ref.c: camera_of). */
static void camera_of(const float *R, const float *p, const float *X, float c[3]) {
    const float d0 = X[0] - p[0], d1 = X[1] - p[1], d2 = X[2] - p[2];
    for (int j = 0; j < 3; ++j) c[j] = (R[j] * d0 + R[3 + j] * d1) + R[6 + j] * d2;
}

static void ray_of(const float *R, float x, float y, float a[3]) {
    a[0] = (R[0] * x + R[1] * y) + R[2];
    a[1] = (R[3] * x + R[4] * y) + R[5];
    a[2] = (R[6] * x + R[7] * y) + R[8];
}

/* Rule c's attempt: the landmark of a slot seen at (ua, va) from the pose pa and at (uc, vc) from the pose pc. */
static int triangulate(const float *K4, float ry, float tn2, float c2, const float *pa, float ua, float va, const float *pc, float uc, float vc, int variant,
                       float X[3]) {
    int finite = finite32(ua) && finite32(va) && finite32(uc) && finite32(vc);
    for (int e = 0; e < 7; ++e) finite = finite && finite32(pa[e]) && finite32(pc[e]);
    if (!finite) return O_FAILS;
    const float fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    const float xa = (ua - cx) / fx, ya = (va - cy) / fy;
    const float xc = (uc - cx) / fx, yc = (vc - cy) / fy;
    float Ra[9], Rc[9], a[3], b[3], t[3];
    rotation_of(pa, Ra);
    rotation_of(pc, Rc);
    ray_of(Ra, xa, ya, a);
    ray_of(Rc, xc, yc, b);
    for (int k = 0; k < 3; ++k) t[k] = variant == T_WITH_THE_OTHER_SIGN ? pc[4 + k] - pa[4 + k] : pa[4 + k] - pc[4 + k];
    /* TwoViewPose's 2 x 2 normal equations of z2 b = z1 a + t (tests/two_view_pose_ref.c) */
    const float aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const float bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    const float ab = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    const float at = (a[0] * t[0] + a[1] * t[1]) + a[2] * t[2];
    const float bt = (b[0] * t[0] + b[1] * t[1]) + b[2] * t[2];
    const float det = aa * bb - ab * ab;
    const float z1 = (ab * bt - bb * at) / det;
    const float z2 = (aa * bt - ab * at) / det;
    if (variant != PARALLAX_TEST_OMITTED && ab * ab > c2 * (aa * bb)) return O_WAITS;
    if (!(finite32(z1) && finite32(z2) && z1 > 0.0f && z2 > 0.0f)) return O_FAILS;
    for (int k = 0; k < 3; ++k) {
        X[k] = variant == ONE_RAY ? pa[4 + k] + z1 * a[k] : ((pa[4 + k] + z1 * a[k]) + (pc[4 + k] + z2 * b[k])) * 0.5f;
    }
    if (!(finite32(X[0]) && finite32(X[1]) && finite32(X[2])) || (X[0] == 0.0f && X[1] == 0.0f && X[2] == 0.0f)) return O_FAILS;
    float ca[3], cc[3];
    camera_of(Ra, pa + 4, X, ca);
    camera_of(Rc, pc + 4, X, cc);
    return inlier(ca[0], ca[1], ca[2], xa, ya, ry, tn2) && inlier(cc[0], cc[1], cc[2], xc, yc, ry, tn2) ? O_KEPT : O_FAILS;
}

int lt_begin(const int64_t *ids, int32_t n, int64_t *owner, float *landmarks, int32_t *anchor_frame, uint8_t *pnp_status, uint8_t *anchor_status,
             int32_t *counters, int32_t variant) {
    counters[C_NEW] = counters[C_ANCHORED] = counters[C_LANDMARKS] = counters[C_DROPPED] = 0;
    for (int32_t s = 0; s < n; ++s) {
        float *L = landmarks + 3 * (size_t)s;
        if (ids[s] != owner[s]) {
            owner[s] = ids[s];
            if (variant != OWNER_CHANGE_KEEPS_LANDMARK) L[0] = L[1] = L[2] = 0.0f;
            anchor_frame[s] = -1;
        }
        const int has = !(L[0] == 0.0f && L[1] == 0.0f && L[2] == 0.0f);
        pnp_status[s] = ids[s] >= 0 && has ? TRACKED : NOT_TRACKED;
        anchor_status[s] = ids[s] >= 0 && anchor_frame[s] >= 0 ? TRACKED : NOT_TRACKED;
    }
    return 0;
}

int lt_end(const int64_t *ids, const float *points, int32_t n, const uint8_t *status_in, const float *pose_in, const int32_t *valid_in,
           const int32_t *model_in, int32_t frame, int32_t mode, const float *K4, float threshold, float c2, float *landmarks, float *anchor_uv,
           float *anchor_pose, int32_t *anchor_frame, int32_t *counters, float *pose, int32_t variant, int8_t *outcome) {
    const int ok = valid_in[0] == 1 && (!model_in || model_in[0] == 0);
    const float ry = K4[1] / K4[0];
    const float tn = threshold / K4[0];
    const float tn2 = tn * tn;
    float pc[7];
    memcpy(pc, pose_in, sizeof pc);
    counters[C_VALID] = ok ? 1 : -1;
    counters[C_LOST] = ok ? 0 : counters[C_LOST] + 1;
    if (ok) memcpy(pose, pc, sizeof pc);
    for (int32_t s = 0; s < n; ++s) {
        if (outcome) outcome[s] = O_NONE;
        if (ids[s] < 0) continue;
        float *L = landmarks + 3 * (size_t)s;
        int holds = !(L[0] == 0.0f && L[1] == 0.0f && L[2] == 0.0f);
        int has_anchor = anchor_frame[s] >= 0;
        counters[C_ANCHORED] += has_anchor;
        if (ok) {
            const int steady = mode == STEADY;
            const float u = points[2 * (size_t)s], v = points[2 * (size_t)s + 1];
            if (steady && status_in[s] == LARGE_RESIDUAL) { /* rule a */
                L[0] = L[1] = L[2] = 0.0f;
                holds = 0, has_anchor = 0;
                counters[C_DROPPED] += 1;
            }
            int anchor_now = steady && !holds && !has_anchor; /* rule b */
            if (!holds && has_anchor && !(variant == RULE_C_OFF && steady)) { /* rule c */
                float X[3] = {0.0f, 0.0f, 0.0f};
                const int o = triangulate(K4, ry, tn2, c2, anchor_pose + 7 * (size_t)s, anchor_uv[2 * (size_t)s], anchor_uv[2 * (size_t)s + 1], pc, u, v, variant, X);
                if (outcome) outcome[s] = (int8_t)o;
                if (o == O_KEPT) {
                    L[0] = X[0], L[1] = X[1], L[2] = X[2];
                    holds = 1;
                    counters[C_NEW] += 1;
                } else if (o == O_FAILS && steady && variant != NO_REANCHOR) {
                    anchor_now = 1;
                }
            }
            if (anchor_now) {
                anchor_uv[2 * (size_t)s] = u, anchor_uv[2 * (size_t)s + 1] = v;
                memcpy(anchor_pose + 7 * (size_t)s, pc, sizeof pc);
                anchor_frame[s] = frame;
            }
        }
        counters[C_LANDMARKS] += holds;
    }
    return 0;
}
