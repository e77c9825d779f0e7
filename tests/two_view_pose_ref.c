/* two_view_pose_ref.c — the scalar CPU restatement of TwoViewPose: relative pose and landmarks from two-view inliers.
 *
 * TEST INFRASTRUCTURE ONLY.  Every float operation of the contract in the order DESIGN.md 5.29 states it, float32, compiled without
 * contraction (tests/ref_build.py's STRICT flags); `/` and sqrtf are correctly rounded.  The device (csrc/two_view_pose_kernels.hip) is held
 * to this file bit for bit by tests/test_two_view_pose_gpu.py; tests/test_two_view_pose_cpu.py pins this file to an independent float64
 * composition, to ground truth and to the projection of DirectMethod.  `variant` 0 is the contract; the others are the mutants that the CPU
 * tests must catch.  `sweeps` is a parameter so that the rule which fixed FTK_POSE_JACOBI_SWEEPS can be asserted.  `trace` (may be NULL)
 * records which way every data-dependent choice went; it reads values the contract computes and changes none of them.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define TRACKED 1
#define LARGE_RESIDUAL 2
#define TILE 256

enum { CONTRACT = 0, TWISTED_PAIR = 1, T_WRONG_SIGN = 2, E_TRANSPOSED = 3, SEQUENTIAL_SUM = 4, REPROJECTION_UNSCALED = 5,
       SHEPPERD_X_SIGN = 6, SHEPPERD_Y_SIGN = 7, SHEPPERD_Z_SIGN = 8, NO_NEGATION = 9 };

/* The trace: 7 choices (-1 where the call ended before making them), then the pairs of the 9 x 9 and of the 3 x 3 Jacobi by the path taken. */
enum { TR_K = 0, TR_K2, TR_I1, TR_I2, TR_WINNER, TR_SHEPPERD, TR_NEGATED, TR_JACOBI9, TR_JACOBI3 = TR_JACOBI9 + 5, TR_LENGTH = TR_JACOBI3 + 5 };
enum { J_ZERO = 0, J_NEGLIGIBLE, J_APQ_OVER_H, J_THETA_POSITIVE, J_THETA_NEGATIVE };

static int finite32(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x7F800000u) != 0x7F800000u;
}

/* Cyclic Jacobi on the symmetric n x n matrix a (full storage, row-major, destroyed; its diagonal ends as the eigenvalues), eigenvectors
 * accumulated in the columns of v.  Pairs (p, q), p < q, in row-major order; `sweeps` sweeps, all of them.  paths (may be NULL) counts the
 * pairs by the path they took. */
static void jacobi_eigen(int n, float *a, float *v, int sweeps, int32_t *paths) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) v[i * n + j] = i == j ? 1.0f : 0.0f;
    for (int sweep = 0; sweep < sweeps; ++sweep) {
        for (int p = 0; p < n - 1; ++p) {
            for (int q = p + 1; q < n; ++q) {
                const float apq = a[p * n + q], app = a[p * n + p], aqq = a[q * n + q];
                if (apq == 0.0f) {
                    if (paths) ++paths[J_ZERO];
                    continue;
                }
                const float g = 100.0f * fabsf(apq);
                if (fabsf(app) + g == fabsf(app) && fabsf(aqq) + g == fabsf(aqq)) { /* negligible: set to zero, no rotation */
                    a[p * n + q] = 0.0f;
                    a[q * n + p] = 0.0f;
                    if (paths) ++paths[J_NEGLIGIBLE];
                    continue;
                }
                const float h = aqq - app;
                float t;
                if (fabsf(h) + g == fabsf(h)) {
                    t = apq / h;
                    if (paths) ++paths[J_APQ_OVER_H];
                } else {
                    const float theta = h / (2.0f * apq);
                    t = 1.0f / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
                    if (theta < 0.0f) t = -t;
                    if (paths) ++paths[theta < 0.0f ? J_THETA_NEGATIVE : J_THETA_POSITIVE];
                }
                const float c = 1.0f / sqrtf(t * t + 1.0f);
                const float s = t * c;
                const float tau = s / (1.0f + c);
                const float hh = t * apq;
                a[p * n + p] = app - hh;
                a[q * n + q] = aqq + hh;
                a[p * n + q] = 0.0f;
                a[q * n + p] = 0.0f;
                for (int r = 0; r < n; ++r) {
                    if (r != p && r != q) {
                        const float x = a[r * n + p], y = a[r * n + q];
                        const float xn = x - s * (y + x * tau), yn = y + s * (x - y * tau);
                        a[r * n + p] = xn;
                        a[p * n + r] = xn;
                        a[r * n + q] = yn;
                        a[q * n + r] = yn;
                    }
                    const float x = v[r * n + p], y = v[r * n + q];
                    v[r * n + p] = x - s * (y + x * tau);
                    v[r * n + q] = y + s * (x - y * tau);
                }
            }
        }
    }
}

/* The two-ray depths of z2 b = z1 a + t (the 2 x 2 normal equations of the midpoint). */
static void depths(const float a[3], const float b[3], const float t[3], float *z1, float *z2) {
    const float aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const float bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    const float ab = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    const float at = (a[0] * t[0] + a[1] * t[1]) + a[2] * t[2];
    const float bt = (b[0] * t[0] + b[1] * t[1]) + b[2] * t[2];
    const float det = aa * bb - ab * ab;
    *z1 = (ab * bt - bb * at) / det;
    *z2 = (aa * bt - ab * at) / det;
}

static void rotate(const float R[9], float x, float y, float a[3]) {
    a[0] = (R[0] * x + R[1] * y) + R[2];
    a[1] = (R[3] * x + R[4] * y) + R[5];
    a[2] = (R[6] * x + R[7] * y) + R[8];
}

static int in_front(const float R[9], const float t[3], const float q[4], float *z1, float *z2) {
    float a[3];
    const float b[3] = {q[2], q[3], 1.0f};
    if (!(finite32(q[0]) && finite32(q[1]) && finite32(q[2]) && finite32(q[3]))) {
        *z1 = *z2 = 0.0f;
        return 0;
    }
    rotate(R, q[0], q[1], a);
    depths(a, b, t, z1, z2);
    return finite32(*z1) && finite32(*z2) && *z1 > 0.0f && *z2 > 0.0f;
}

/* K8 = (fx, fy, cx, cy) of the reference view, then of the current view.  a45 (may be NULL) receives the 45 sums, trace (may be NULL) the
 * TR_LENGTH entries of the trace. */
int tvp_solve(const float *ref_uv, const float *cur_uv, uint8_t *status, int32_t n, const float *K8, float threshold, float baseline, int32_t sweeps,
              int32_t variant, float *pose, float *points, float *E_out, int32_t *n_front, int32_t *valid, int32_t *n_points, float *a45,
              int32_t *trace) {
    if (n < 1 || n > 65536 || sweeps < 0) return -1;
    static float pts[65536][4];
    const float fx1 = K8[0], fy1 = K8[1], cx1 = K8[2], cy1 = K8[3], fx2 = K8[4], fy2 = K8[5], cx2 = K8[6], cy2 = K8[7];
    const float t2 = threshold * threshold;
    /* 1. the participants, ascending, with their calibrated coordinates */
    int32_t m = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (status[i] == TRACKED) {
            pts[m][0] = (ref_uv[2 * i] - cx1) / fx1;
            pts[m][1] = (ref_uv[2 * i + 1] - cy1) / fy1;
            pts[m][2] = (cur_uv[2 * i] - cx2) / fx2;
            pts[m][3] = (cur_uv[2 * i + 1] - cy2) / fy2;
            ++m;
        }
    }
    /* the invalid result; what follows overwrites it */
    memset(points, 0, sizeof(float) * 3 * (size_t)n);
    memset(E_out, 0, sizeof(float) * 9);
    memset(pose, 0, sizeof(float) * 7);
    pose[0] = 1.0f;
    memset(n_front, 0, sizeof(int32_t) * 4);
    *valid = -1;
    *n_points = 0;
    if (a45) memset(a45, 0, sizeof(float) * 45);
    if (trace) {
        for (int i = 0; i < TR_JACOBI9; ++i) trace[i] = -1;
        for (int i = TR_JACOBI9; i < TR_LENGTH; ++i) trace[i] = 0;
    }
    if (m < 8) return 0;
    /* 2. the 45 sums: tiles of 256 positions, a tree within the tile, tile totals in ascending order from +0 */
    float sums[45];
    for (int e = 0; e < 45; ++e) sums[e] = 0.0f;
    const int tiles = (m + TILE - 1) / TILE;
    static float tree[45][TILE];
    for (int tile = 0; tile < tiles; ++tile) {
        for (int j = 0; j < TILE; ++j) {
            const int k = tile * TILE + j;
            float r[9];
            int use = k < m;
            if (use) {
                const float x1 = pts[k][0], y1 = pts[k][1], x2 = pts[k][2], y2 = pts[k][3];
                use = finite32(x1) && finite32(y1) && finite32(x2) && finite32(y2);
                r[0] = x2 * x1, r[1] = x2 * y1, r[2] = x2, r[3] = y2 * x1, r[4] = y2 * y1, r[5] = y2, r[6] = x1, r[7] = y1, r[8] = 1.0f;
            }
            int e = 0;
            for (int a = 0; a < 9; ++a)
                for (int b = a; b < 9; ++b, ++e) tree[e][j] = use ? r[a] * r[b] : 0.0f;
        }
        for (int e = 0; e < 45; ++e) {
            if (variant == SEQUENTIAL_SUM) {
                float acc = 0.0f;
                for (int j = 0; j < TILE; ++j) acc = acc + tree[e][j];
                tree[e][0] = acc;
            } else {
                for (int stride = TILE / 2; stride >= 1; stride >>= 1)
                    for (int j = 0; j < stride; ++j) tree[e][j] = tree[e][j] + tree[e][j + stride];
            }
            sums[e] = sums[e] + tree[e][0];
        }
    }
    if (a45) memcpy(a45, sums, sizeof(sums));
    /* 3. the null vector: the eigenvector of the smallest eigenvalue, ties to the lowest column */
    float A[81], V[81];
    {
        int e = 0;
        for (int a = 0; a < 9; ++a)
            for (int b = a; b < 9; ++b, ++e) A[a * 9 + b] = A[b * 9 + a] = sums[e];
    }
    jacobi_eigen(9, A, V, sweeps, trace ? trace + TR_JACOBI9 : 0);
    int k = 0;
    for (int j = 1; j < 9; ++j)
        if (A[j * 9 + j] < A[k * 9 + k]) k = j;
    /* the rank test: the second-smallest eigenvalue (ties to the lowest column) must exceed 2^-20 of the largest, else the null space has
     * more than one dimension in float32 and the null vector is not determined */
    int k2 = k == 0 ? 1 : 0;
    float lmax = A[0];
    for (int j = 1; j < 9; ++j) {
        if (j != k && A[j * 9 + j] < A[k2 * 9 + k2]) k2 = j;
        if (A[j * 9 + j] > lmax) lmax = A[j * 9 + j];
    }
    const int rank_ok = A[k2 * 9 + k2] > 9.5367431640625e-07f * lmax;
    float E[9];
    for (int i = 0; i < 9; ++i) E[i] = V[i * 9 + k];
    if (variant == E_TRANSPOSED) {
        float T[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) T[i * 3 + j] = E[j * 3 + i];
        memcpy(E, T, sizeof(E));
    }
    /* 4. the essential projection and the four candidates */
    float G[9], W[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) G[i * 3 + j] = (E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j];
    jacobi_eigen(3, G, W, sweeps, trace ? trace + TR_JACOBI3 : 0);
    const float l0 = G[0], l1 = G[4], l2 = G[8];
    int i1 = 0;
    if (l1 > l0) i1 = 1;
    if (l2 > (i1 == 0 ? l0 : l1)) i1 = 2;
    const int ia = i1 == 0 ? 1 : 0, ib = i1 == 2 ? 1 : 2; /* the other two, ascending */
    const int i2 = G[ib * 4] > G[ia * 4] ? ib : ia;
    if (trace) trace[TR_K] = k, trace[TR_K2] = k2, trace[TR_I1] = i1, trace[TR_I2] = i2;
    const float s1 = sqrtf(G[i1 * 4]), s2 = sqrtf(G[i2 * 4]);
    float v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
    for (int i = 0; i < 3; ++i) v1[i] = W[i * 3 + i1], v2[i] = W[i * 3 + i2];
    for (int i = 0; i < 3; ++i) {
        u1[i] = ((E[i * 3] * v1[0] + E[i * 3 + 1] * v1[1]) + E[i * 3 + 2] * v1[2]) / s1;
        u2[i] = ((E[i * 3] * v2[0] + E[i * 3 + 1] * v2[1]) + E[i * 3 + 2] * v2[2]) / s2;
    }
    v3[0] = v1[1] * v2[2] - v1[2] * v2[1], v3[1] = v1[2] * v2[0] - v1[0] * v2[2], v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1], u3[1] = u1[2] * u2[0] - u1[0] * u2[2], u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    float Eh[9], Ra[9], Rb[9];
    int ok = rank_ok;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Eh[i * 3 + j] = u1[i] * v1[j] + u2[i] * v2[j];
            Ra[i * 3 + j] = (u2[i] * v1[j] - u1[i] * v2[j]) + u3[i] * v3[j];
            Rb[i * 3 + j] = (u1[i] * v2[j] - u2[i] * v1[j]) + u3[i] * v3[j];
            ok = ok && finite32(Eh[i * 3 + j]) && finite32(Ra[i * 3 + j]) && finite32(Rb[i * 3 + j]);
        }
    for (int i = 0; i < 3; ++i) ok = ok && finite32(u3[i]);
    if (!ok) return 0;
    /* 5. cheirality: candidate c = 2 * (R is Rb) + (t is -u3) */
    const float tm[3] = {-u3[0], -u3[1], -u3[2]};
    for (int c = 0; c < 4; ++c) {
        const float *R = c < 2 ? Ra : Rb, *t = (c & 1) ? tm : u3;
        for (int j = 0; j < m; ++j) {
            float z1, z2;
            n_front[c] += in_front(R, t, pts[j], &z1, &z2);
        }
    }
    int win = 0;
    for (int c = 1; c < 4; ++c)
        if (n_front[c] > n_front[win]) win = c;
    if (n_front[win] <= 0) return 0;
    if (trace) trace[TR_WINNER] = win;
    /* 6. the pose in DirectMethod's convention: R_rc = R^T, p_rc = -R^T t scaled to the baseline */
    int out = win;
    if (variant == TWISTED_PAIR) out = win ^ 2;
    const float *R = out < 2 ? Ra : Rb, *t = (out & 1) ? tm : u3;
    const float nt = sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    const float sc = baseline / nt;
    float ts[3] = {t[0] * sc, t[1] * sc, t[2] * sc};
    if (variant == T_WRONG_SIGN) ts[0] = -ts[0], ts[1] = -ts[1], ts[2] = -ts[2];
    float ps[7];
    for (int j = 0; j < 3; ++j) ps[4 + j] = -((R[j] * ts[0] + R[3 + j] * ts[1]) + R[6 + j] * ts[2]);
    /* Shepperd on M = R^T: M(i, j) = R[j * 3 + i] */
    const float m00 = R[0], m01 = R[3], m02 = R[6], m10 = R[1], m11 = R[4], m12 = R[7], m20 = R[2], m21 = R[5], m22 = R[8];
    const float tr = (m00 + m11) + m22;
    float qw, qx, qy, qz;
    int branch = 0;
    if (tr > 0.0f) {
        const float s = sqrtf(tr + 1.0f) * 2.0f;
        qw = 0.25f * s, qx = (m21 - m12) / s, qy = (m02 - m20) / s, qz = (m10 - m01) / s;
    } else if (m00 > m11 && m00 > m22) {
        const float s = sqrtf(((1.0f + m00) - m11) - m22) * 2.0f;
        qw = (m21 - m12) / s, qx = 0.25f * s, qy = (m01 + m10) / s, qz = (m02 + m20) / s;
        if (variant == SHEPPERD_X_SIGN) qy = (m01 - m10) / s;
        branch = 1;
    } else if (m11 > m22) {
        const float s = sqrtf(((1.0f + m11) - m00) - m22) * 2.0f;
        qw = (m02 - m20) / s, qx = (m01 + m10) / s, qy = 0.25f * s, qz = (m12 + m21) / s;
        if (variant == SHEPPERD_Y_SIGN) qz = (m12 - m21) / s;
        branch = 2;
    } else {
        const float s = sqrtf(((1.0f + m22) - m00) - m11) * 2.0f;
        qw = (m10 - m01) / s, qx = (m02 + m20) / s, qy = (m12 + m21) / s, qz = 0.25f * s;
        if (variant == SHEPPERD_Z_SIGN) qx = (m02 - m20) / s;
        branch = 3;
    }
    const int negate = qw < 0.0f;
    if (negate && variant != NO_NEGATION) qw = -qw, qx = -qx, qy = -qy, qz = -qz;
    if (trace) trace[TR_SHEPPERD] = branch, trace[TR_NEGATED] = negate;
    const float qn = sqrtf(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    ps[0] = qw / qn, ps[1] = qx / qn, ps[2] = qy / qn, ps[3] = qz / qn;
    for (int i = 0; i < 7; ++i) ok = ok && finite32(ps[i]);
    if (!ok) return 0;
    *valid = 1;
    memcpy(pose, ps, sizeof(ps));
    memcpy(E_out, Eh, sizeof(Eh));
    /* the landmarks and the statuses (the winner's R and t, whatever a mutant put into the pose) */
    const float *Rw = win < 2 ? Ra : Rb, *tw = (win & 1) ? tm : u3;
    int32_t j = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (status[i] != TRACKED) continue;
        const float *q = pts[j++];
        float z1, z2;
        int keep = in_front(Rw, tw, q, &z1, &z2);
        if (keep) {
            float a[3];
            rotate(Rw, q[0], q[1], a);
            const float X = z1 * a[0] + tw[0], Y = z1 * a[1] + tw[1], Z = z1 * a[2] + tw[2];
            float ex = X - q[2] * Z, ey = Y - q[3] * Z;
            if (variant != REPROJECTION_UNSCALED) ex = fx2 * ex, ey = fy2 * ey;
            const float lhs = ex * ex + ey * ey, rhs = t2 * (Z * Z);
            keep = finite32(lhs) && finite32(rhs) && lhs <= rhs;
        }
        if (keep) {
            const float zs = z1 * sc;
            points[3 * i] = zs * q[0], points[3 * i + 1] = zs * q[1], points[3 * i + 2] = zs;
            ++*n_points;
        } else {
            status[i] = LARGE_RESIDUAL;
        }
    }
    return 0;
}
