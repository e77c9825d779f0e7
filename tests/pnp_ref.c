/* pnp_ref.c — the scalar CPU restatement of PnpRansac: the camera pose from landmarks and their pixels, RANSAC over the
 * six-point DLT and a Gauss-Newton refit of the reprojection error on the inliers.
 *
 * TEST INFRASTRUCTURE ONLY.  Every float operation of the contract in the order DESIGN.md 5.30 states it, float32, compiled without
 * contraction (tests/ref_build.py's STRICT flags); `/` and sqrtf are correctly rounded.  The device (csrc/pnp_kernels.hip) is held to this
 * file bit for bit by tests/test_pnp_gpu.py; tests/test_pnp_cpu.py pins this file to an independent float64 restatement (tests/pnp_ref64.py)
 * and to ground truth.  `variant` 0 is the contract; the others are the mutants that the CPU tests must catch.  `trace` (may be NULL)
 * records which way every data-dependent choice went; it reads values the contract computes and changes none of them.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { TRACKED = 1, LARGE_RESIDUAL = 2, SAMPLE = 6, ATTEMPTS = 16, TILE = 256, ROWS = 11, COLS = 12, SUMS = 27, SWEEPS = 7, MAX_STEPS = 16 };
enum { CONTRACT = 0, SIGN_NOT_FIXED = 1, A_TRANSPOSED = 2, SEQUENTIAL_SUM = 3, Y_UNSCALED = 4, ZERO_RULE_OMITTED = 5 };
/* The trace: the winner, the quaternion's branch, the negation after it, the sign of det A (1: negative), the negation at the end, the
 * number of accepted refit steps, then each step's outcome (-1: not reached). */
enum { TR_WINNER = 0, TR_SHEPPERD, TR_NEGATED, TR_DET_NEGATIVE, TR_FINAL_NEGATED, TR_STEPS, TR_STEP0, TR_LENGTH = TR_STEP0 + MAX_STEPS };
enum { STEP_TAKEN = 0, STEP_FEW_INLIERS = 1, STEP_NOT_POSITIVE_DEFINITE = 2, STEP_NOT_FINITE = 3 };

static int finite32(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x7F800000u) != 0x7F800000u;
}

static uint32_t fmix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

static uint32_t mix32(uint32_t seed, uint32_t h, uint32_t k, uint32_t a) {
    return fmix32(fmix32(seed + 0x9E3779B9u * (h + 1u)) ^ (0x85EBCA6Bu * (k * (uint32_t)ATTEMPTS + a + 1u)));
}

/* A participant: the calibrated pixel (x, y) and the landmark (X, Y, Z). */
typedef struct { float x, y, X, Y, Z; } Part;

/* The inlier rule on camera coordinates (c0, c1, c2) of a landmark: in front, and the squared calibrated reprojection error, its y part
 * scaled by ry = fy / fx, at most tn2 = (threshold / fx)^2; without the division. */
static int inlier(float c0, float c1, float c2, float x, float y, float ry, float tn2) {
    const float ex = c0 - x * c2;
    const float ey = (c1 - y * c2) * ry;
    const float lhs = ex * ex + ey * ey, rhs = tn2 * (c2 * c2);
    return c2 > 0.0f && finite32(lhs) && finite32(rhs) && lhs <= rhs;
}

/* Camera coordinates under a 3 x 4 model P (row-major). */
static void project(const float *P, const Part *q, float c[3]) {
    for (int r = 0; r < 3; ++r) c[r] = ((P[r * 4] * q->X + P[r * 4 + 1] * q->Y) + P[r * 4 + 2] * q->Z) + P[r * 4 + 3];
}

/* The unit null vector of the ROWS x COLS matrix a by Gaussian elimination with complete pivoting (the first maximum in row-major order),
 * back substitution with the free unknown 1 and scaling to unit norm: the two-view filters' elimination at 11 x 12.  0: invalid. */
static int null_vector(float a[ROWS][COLS], float *f) {
    int perm[COLS];
    for (int c = 0; c < COLS; ++c) perm[c] = c;
    for (int s = 0; s < ROWS; ++s) {
        float best = -1.0f;
        int br = s, bc = s;
        for (int r = s; r < ROWS; ++r) {
            for (int c = s; c < COLS; ++c) {
                const float v = fabsf(a[r][c]);
                if (v > best) best = v, br = r, bc = c;
            }
        }
        const float piv = a[br][bc];
        if (!finite32(piv) || piv == 0.0f) return 0;
        for (int c = 0; c < COLS; ++c) {
            const float t = a[s][c];
            a[s][c] = a[br][c];
            a[br][c] = t;
        }
        for (int r = 0; r < ROWS; ++r) {
            const float t = a[r][s];
            a[r][s] = a[r][bc];
            a[r][bc] = t;
        }
        const int t = perm[s];
        perm[s] = perm[bc];
        perm[bc] = t;
        for (int r = s + 1; r < ROWS; ++r) {
            const float mult = a[r][s] / piv;
            for (int c = s + 1; c < COLS; ++c) a[r][c] = a[r][c] - mult * a[s][c];
        }
    }
    float z[COLS], v[COLS];
    z[COLS - 1] = 1.0f;
    for (int s = ROWS - 1; s >= 0; --s) {
        float acc = a[s][COLS - 1];
        for (int c = s + 1; c < ROWS; ++c) acc = acc + a[s][c] * z[c];
        z[s] = -acc / a[s][s];
    }
    for (int c = 0; c < COLS; ++c) v[perm[c]] = z[c];
    float n2 = v[0] * v[0];
    for (int i = 1; i < COLS; ++i) n2 = n2 + v[i] * v[i];
    if (!(finite32(n2) && n2 > 0.0f)) return 0;
    const float inv = 1.0f / sqrtf(n2);
    int ok = 1;
    for (int i = 0; i < COLS; ++i) {
        f[i] = v[i] * inv;
        ok = ok && finite32(f[i]);
    }
    return ok;
}

/* One hypothesis: the 3 x 4 model P = [A | b] of six participants (x_cur ~ A X + b), 0 = invalid. */
static int fit(const Part *q[SAMPLE], int variant, float *P) {
    /* conditioning from the sample alone: the mean in index order, the mean absolute deviation over the 18 coordinates */
    float mean[3];
    mean[0] = (((((q[0]->X + q[1]->X) + q[2]->X) + q[3]->X) + q[4]->X) + q[5]->X) / 6.0f;
    mean[1] = (((((q[0]->Y + q[1]->Y) + q[2]->Y) + q[3]->Y) + q[4]->Y) + q[5]->Y) / 6.0f;
    mean[2] = (((((q[0]->Z + q[1]->Z) + q[2]->Z) + q[3]->Z) + q[4]->Z) + q[5]->Z) / 6.0f;
    float dev = 0.0f, c[SAMPLE][3];
    for (int k = 0; k < SAMPLE; ++k) {
        c[k][0] = q[k]->X - mean[0], c[k][1] = q[k]->Y - mean[1], c[k][2] = q[k]->Z - mean[2];
        const float d = (fabsf(c[k][0]) + fabsf(c[k][1])) + fabsf(c[k][2]);
        dev = k == 0 ? d : dev + d;
    }
    const float s = dev / 18.0f;
    if (!(finite32(s) && s > 0.0f)) return 0;
    float a[ROWS + 1][COLS];
    for (int k = 0; k < SAMPLE; ++k) {
        const float X = c[k][0] / s, Y = c[k][1] / s, Z = c[k][2] / s, x = q[k]->x, y = q[k]->y;
        const float r0[COLS] = {X, Y, Z, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, -(x * X), -(x * Y), -(x * Z), -x};
        const float r1[COLS] = {0.0f, 0.0f, 0.0f, 0.0f, X, Y, Z, 1.0f, -(y * X), -(y * Y), -(y * Z), -y};
        memcpy(a[2 * k], r0, sizeof(r0));
        memcpy(a[2 * k + 1], r1, sizeof(r1)); /* (the twelfth row is not used) */
    }
    float f[COLS];
    if (!null_vector(a, f)) return 0;
    /* the conditioning folded back, times s: A = the normalised A, b = s b_n - A mean */
    for (int r = 0; r < 3; ++r) {
        P[r * 4] = f[r * 4], P[r * 4 + 1] = f[r * 4 + 1], P[r * 4 + 2] = f[r * 4 + 2];
        P[r * 4 + 3] = s * f[r * 4 + 3] - ((f[r * 4] * mean[0] + f[r * 4 + 1] * mean[1]) + f[r * 4 + 2] * mean[2]);
    }
    /* the sign: the sample's depths positive */
    int front = 0, behind = 0;
    for (int k = 0; k < SAMPLE; ++k) {
        const float w = ((P[8] * q[k]->X + P[9] * q[k]->Y) + P[10] * q[k]->Z) + P[11];
        front += w > 0.0f;
        behind += w < 0.0f;
    }
    if (front != SAMPLE && behind != SAMPLE) return 0;
    if (behind == SAMPLE && variant != SIGN_NOT_FIXED) {
        for (int i = 0; i < 12; ++i) P[i] = -P[i];
    }
    for (int i = 0; i < 12; ++i) {
        if (!finite32(P[i])) return 0;
    }
    return 1;
}

/* Cyclic Jacobi on the symmetric 3 x 3 matrix a (full storage, row-major; its diagonal ends as the eigenvalues), eigenvectors in the columns of
 * v: TwoViewPose's solver (tests/two_view_pose_ref.c), pairs (p, q), p < q, in row-major order, SWEEPS sweeps, all of them. */
static void jacobi3(float *a, float *v) {
    const int n = 3;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) v[i * n + j] = i == j ? 1.0f : 0.0f;
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        for (int p = 0; p < n - 1; ++p) {
            for (int q = p + 1; q < n; ++q) {
                const float apq = a[p * n + q], app = a[p * n + p], aqq = a[q * n + q];
                if (apq == 0.0f) continue;
                const float g = 100.0f * fabsf(apq);
                if (fabsf(app) + g == fabsf(app) && fabsf(aqq) + g == fabsf(aqq)) {
                    a[p * n + q] = 0.0f;
                    a[q * n + p] = 0.0f;
                    continue;
                }
                const float h = aqq - app;
                float t;
                if (fabsf(h) + g == fabsf(h)) {
                    t = apq / h;
                } else {
                    const float theta = h / (2.0f * apq);
                    t = 1.0f / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
                    if (theta < 0.0f) t = -t;
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

/* The winner's P = [A | b] as a pose (q_rc, p_rc): R the nearest rotation to A, t = b / s with s the mean singular value; R_rc = R^T,
 * p_rc = -R^T t.  0: not finite or singular. */
static int pose_of_model(const float *P, int variant, float *pose, int32_t *trace) {
    float A[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) A[r * 3 + c] = variant == A_TRANSPOSED ? P[c * 4 + r] : P[r * 4 + c];
    float M[9], V[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i * 3 + j] = (A[i] * A[j] + A[3 + i] * A[3 + j]) + A[6 + i] * A[6 + j];
    jacobi3(M, V);
    const float l0 = M[0], l1 = M[4], l2 = M[8];
    if (!(l0 > 0.0f && l1 > 0.0f && l2 > 0.0f)) return 0;
    const float sg[3] = {sqrtf(l0), sqrtf(l1), sqrtf(l2)};
    const float det = (A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])) + A[2] * (A[3] * A[7] - A[4] * A[6]);
    if (!finite32(det) || det == 0.0f) return 0;
    /* det < 0: the term of the smallest eigenvalue (the lowest index among equals) enters with the other sign */
    int small = 0;
    if (M[4] < M[small * 4]) small = 1;
    if (M[8] < M[small * 4]) small = 2;
    float w[3];
    for (int k = 0; k < 3; ++k) w[k] = 1.0f / sg[k];
    if (det < 0.0f) w[small] = -w[small];
    if (trace) trace[TR_DET_NEGATIVE] = det < 0.0f;
    /* R = A W, W = V diag(w) V^T */
    float W[9], R[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W[i * 3 + j] = ((V[i * 3] * w[0]) * V[j * 3] + (V[i * 3 + 1] * w[1]) * V[j * 3 + 1]) + (V[i * 3 + 2] * w[2]) * V[j * 3 + 2];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = (A[i * 3] * W[j] + A[i * 3 + 1] * W[3 + j]) + A[i * 3 + 2] * W[6 + j];
    const float sc = ((sg[0] + sg[1]) + sg[2]) / 3.0f;
    const float t0 = P[3] / sc, t1 = P[7] / sc, t2 = P[11] / sc;
    for (int j = 0; j < 3; ++j) pose[4 + j] = -((R[j] * t0 + R[3 + j] * t1) + R[6 + j] * t2);
    /* Shepperd on R_rc = R^T: m(i, j) = R[j * 3 + i], as TwoViewPose */
    const float m00 = R[0], m01 = R[3], m02 = R[6], m10 = R[1], m11 = R[4], m12 = R[7], m20 = R[2], m21 = R[5], m22 = R[8];
    const float tr = (m00 + m11) + m22;
    float qw, qx, qy, qz;
    int branch;
    if (tr > 0.0f) {
        const float s = sqrtf(tr + 1.0f) * 2.0f;
        qw = 0.25f * s, qx = (m21 - m12) / s, qy = (m02 - m20) / s, qz = (m10 - m01) / s, branch = 0;
    } else if (m00 > m11 && m00 > m22) {
        const float s = sqrtf(((1.0f + m00) - m11) - m22) * 2.0f;
        qw = (m21 - m12) / s, qx = 0.25f * s, qy = (m01 + m10) / s, qz = (m02 + m20) / s, branch = 1;
    } else if (m11 > m22) {
        const float s = sqrtf(((1.0f + m11) - m00) - m22) * 2.0f;
        qw = (m02 - m20) / s, qx = (m01 + m10) / s, qy = 0.25f * s, qz = (m12 + m21) / s, branch = 2;
    } else {
        const float s = sqrtf(((1.0f + m22) - m00) - m11) * 2.0f;
        qw = (m10 - m01) / s, qx = (m02 + m20) / s, qy = (m12 + m21) / s, qz = 0.25f * s, branch = 3;
    }
    const int negated = qw < 0.0f;
    if (negated) qw = -qw, qx = -qx, qy = -qy, qz = -qz;
    const float qn = sqrtf(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    pose[0] = qw / qn, pose[1] = qx / qn, pose[2] = qy / qn, pose[3] = qz / qn;
    for (int e = 0; e < 7; ++e) {
        if (!finite32(pose[e])) return 0;
    }
    if (trace) trace[TR_SHEPPERD] = branch, trace[TR_NEGATED] = negated;
    return 1;
}

/* R_rc of a unit quaternion (w, x, y, z), row-major. */
static void rotation_of(const float *q, float *R) {
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0f - 2.0f * (y * y + z * z), R[1] = 2.0f * (x * y - w * z), R[2] = 2.0f * (x * z + w * y);
    R[3] = 2.0f * (x * y + w * z), R[4] = 1.0f - 2.0f * (x * x + z * z), R[5] = 2.0f * (y * z - w * x);
    R[6] = 2.0f * (x * z - w * y), R[7] = 2.0f * (y * z + w * x), R[8] = 1.0f - 2.0f * (x * x + y * y);
}

/* Camera coordinates under a pose: c = R_rc^T (X - p_rc). */
static void camera_of(const float *R, const float *p, const Part *q, float c[3]) {
    const float d0 = q->X - p[0], d1 = q->Y - p[1], d2 = q->Z - p[2];
    for (int j = 0; j < 3; ++j) c[j] = (R[j] * d0 + R[3 + j] * d1) + R[6 + j] * d2;
}

/* A participant's 27 terms of the normal equations under a pose (zeros when it is not taken): the 21 entries of J^T J, upper triangle in
 * row-major order, then the 6 of J^T r.  Taken: an inlier of the pose; at the first step (P, the winner's model, not NULL) an inlier of P
 * that lies in front of the camera under the pose.  Returns whether it is taken. */
static int terms_of(const float *R, const float *p, const float *P, const Part *q, float ry, float tn2, float *term) {
    float c[3];
    camera_of(R, p, q, c);
    memset(term, 0, sizeof(float) * SUMS);
    if (P) {
        float cp[3];
        project(P, q, cp);
        if (!(inlier(cp[0], cp[1], cp[2], q->x, q->y, ry, tn2) && c[2] > 0.0f)) return 0;
    } else if (!inlier(c[0], c[1], c[2], q->x, q->y, ry, tn2)) {
        return 0;
    }
    const float iz = 1.0f / c[2];
    const float a = c[0] * iz, b = c[1] * iz;
    const float j1[6] = {a * b, -(1.0f + a * a), b, -iz, 0.0f, a * iz};
    const float j2[6] = {ry * (1.0f + b * b), ry * -(a * b), ry * -a, 0.0f, ry * -iz, ry * (b * iz)};
    const float r1 = a - q->x, r2 = (b - q->y) * ry;
    int e = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) term[e++] = j1[i] * j1[j] + j2[i] * j2[j];
    for (int i = 0; i < 6; ++i) term[e++] = j1[i] * r1 + j2[i] * r2;
    return 1;
}

/* H x = -g by an LDL^T without pivoting, column by column; 0: a pivot is not > 0 (H is not positive definite) or not finite. */
static int ldlt6(const float *sums, float *x) {
    float H[6][6], L[6][6], d[6], y[6];
    int e = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) H[i][j] = H[j][i] = sums[e++];
    for (int j = 0; j < 6; ++j) {
        float acc = H[j][j];
        for (int k = 0; k < j; ++k) acc = acc - (L[j][k] * L[j][k]) * d[k];
        if (!(finite32(acc) && acc > 0.0f)) return 0;
        d[j] = acc;
        for (int i = j + 1; i < 6; ++i) {
            float v = H[i][j];
            for (int k = 0; k < j; ++k) v = v - (L[i][k] * L[j][k]) * d[k];
            L[i][j] = v / acc;
        }
    }
    for (int i = 0; i < 6; ++i) {
        float v = -sums[21 + i];
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v;
    }
    for (int i = 0; i < 6; ++i) y[i] = y[i] / d[i];
    for (int i = 5; i >= 0; --i) {
        float v = y[i];
        for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * x[k];
        x[i] = v;
    }
    return 1;
}

/* K4 = (fx, fy, cx, cy).  counts [hypotheses], models [hypotheses][12], sums27 (the first refit step's 27 sums) and trace may be NULL. */
int pnp_solve(const float *landmarks, const float *uv, uint8_t *status, int32_t n, const float *K4, float threshold, int32_t hypotheses,
              uint32_t seed, int32_t refine, int32_t variant, float *pose, int32_t *n_inliers, int32_t *best_out, int32_t *valid,
              int32_t *counts_out, float *models_out, float *sums27, int32_t *trace) {
    if (n < 1 || n > 65536 || hypotheses < 1 || hypotheses > 4096 || refine < 0 || refine > MAX_STEPS) return -1;
    const float fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    const float tn = threshold / fx, tn2 = tn * tn;
    const float ry = variant == Y_UNSCALED ? 1.0f : fy / fx;
    Part *part = malloc(sizeof(Part) * (size_t)n);
    int32_t *list = malloc(sizeof(int32_t) * (size_t)n);
    int32_t *counts = malloc(sizeof(int32_t) * (size_t)hypotheses);
    float *models = malloc(sizeof(float) * 12 * (size_t)hypotheses);
    float(*tree)[TILE] = malloc(sizeof(float) * SUMS * TILE);
    /* the invalid result; what follows overwrites it */
    pose[0] = 1.0f;
    for (int e = 1; e < 7; ++e) pose[e] = 0.0f;
    n_inliers[0] = 0, best_out[0] = -1, valid[0] = -1;
    if (trace) {
        for (int e = 0; e < TR_LENGTH; ++e) trace[e] = -1;
    }
    if (sums27) memset(sums27, 0, sizeof(float) * SUMS);
    /* 1. the participants, ascending */
    int32_t m = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (status[i] != TRACKED) continue;
        const float X = landmarks[3 * i], Y = landmarks[3 * i + 1], Z = landmarks[3 * i + 2], u = uv[2 * i], v = uv[2 * i + 1];
        if (!(finite32(X) && finite32(Y) && finite32(Z) && finite32(u) && finite32(v))) continue;
        if (X == 0.0f && Y == 0.0f && Z == 0.0f && variant != ZERO_RULE_OMITTED) continue;
        part[m].x = (u - cx) / fx, part[m].y = (v - cy) / fy, part[m].X = X, part[m].Y = Y, part[m].Z = Z;
        list[m++] = i;
    }
    /* 2., 3. the hypotheses and their counts; 4. the winner: the highest count, the lowest index among equals */
    int32_t best = -1, best_count = -1;
    for (int32_t h = 0; h < hypotheses; ++h) {
        uint32_t idx[SAMPLE];
        int ok = m >= SAMPLE;
        for (int k = 0; k < SAMPLE; ++k) {
            int found = 0;
            for (uint32_t t = 0; ok && !found && t < ATTEMPTS; ++t) {
                const uint32_t j = (uint32_t)(((uint64_t)mix32(seed, (uint32_t)h, (uint32_t)k, t) * (uint64_t)m) >> 32);
                int dup = 0;
                for (int e = 0; e < k; ++e) dup = dup || idx[e] == j;
                if (!dup) idx[k] = j, found = 1;
            }
            ok = ok && found;
        }
        float *P = models + 12 * (size_t)h;
        if (ok) {
            const Part *q[SAMPLE];
            for (int k = 0; k < SAMPLE; ++k) q[k] = part + idx[k];
            ok = fit(q, variant, P);
        }
        if (!ok) {
            memset(P, 0, sizeof(float) * 12);
            counts[h] = -1;
            continue;
        }
        int32_t count = 0;
        for (int32_t j = 0; j < m; ++j) {
            float c[3];
            project(P, part + j, c);
            count += inlier(c[0], c[1], c[2], part[j].x, part[j].y, ry, tn2);
        }
        counts[h] = count;
        if (count > best_count) best_count = count, best = h;
    }
    if (counts_out) memcpy(counts_out, counts, sizeof(int32_t) * (size_t)hypotheses);
    if (models_out) memcpy(models_out, models, sizeof(float) * 12 * (size_t)hypotheses);
    float ps[7];
    int ok = best >= 0 && pose_of_model(models + 12 * (size_t)(best < 0 ? 0 : best), variant, ps, trace);
    if (ok && trace) trace[TR_WINNER] = best, trace[TR_STEPS] = 0;
    /* 5. the refit */
    for (int step = 0; ok && step < refine; ++step) {
        float R[9], sums[SUMS], term[SUMS];
        rotation_of(ps, R);
        const float *first = step == 0 ? models + 12 * (size_t)best : NULL; /* the first step refits on the inliers of the model that won */
        int32_t count = 0;
        for (int e = 0; e < SUMS; ++e) sums[e] = 0.0f;
        if (variant == SEQUENTIAL_SUM) {
            for (int32_t j = 0; j < m; ++j) {
                count += terms_of(R, ps + 4, first, part + j, ry, tn2, term);
                for (int e = 0; e < SUMS; ++e) sums[e] = sums[e] + term[e];
            }
        } else {
            for (int32_t base = 0; base < m; base += TILE) { /* tiles of 256 by the tree p[j] += p[j + stride], then the tiles in order */
                for (int j = 0; j < TILE; ++j) {
                    memset(term, 0, sizeof(term));
                    if (base + j < m) count += terms_of(R, ps + 4, first, part + base + j, ry, tn2, term);
                    for (int e = 0; e < SUMS; ++e) tree[e][j] = term[e];
                }
                for (int stride = TILE / 2; stride >= 1; stride >>= 1)
                    for (int e = 0; e < SUMS; ++e)
                        for (int j = 0; j < stride; ++j) tree[e][j] = tree[e][j] + tree[e][j + stride];
                for (int e = 0; e < SUMS; ++e) sums[e] = sums[e] + tree[e][0];
            }
        }
        if (step == 0 && sums27) memcpy(sums27, sums, sizeof(sums));
        int outcome = STEP_TAKEN;
        float dx[6], nq[4], np[3];
        if (count < SAMPLE) {
            outcome = STEP_FEW_INLIERS;
        } else if (!ldlt6(sums, dx)) {
            outcome = STEP_NOT_POSITIVE_DEFINITE;
        } else {
            /* q <- q (1, dtheta / 2), renormalised; p <- p + R_rc dt */
            const float w = ps[0], x = ps[1], y = ps[2], z = ps[3], hx = 0.5f * dx[0], hy = 0.5f * dx[1], hz = 0.5f * dx[2];
            nq[0] = ((w - x * hx) - y * hy) - z * hz;
            nq[1] = ((x + w * hx) + y * hz) - z * hy;
            nq[2] = ((y + w * hy) + z * hx) - x * hz;
            nq[3] = ((z + w * hz) + x * hy) - y * hx;
            const float qn = sqrtf(((nq[0] * nq[0] + nq[1] * nq[1]) + nq[2] * nq[2]) + nq[3] * nq[3]);
            for (int e = 0; e < 4; ++e) nq[e] = nq[e] / qn;
            for (int i = 0; i < 3; ++i) np[i] = ps[4 + i] + ((R[i * 3] * dx[3] + R[i * 3 + 1] * dx[4]) + R[i * 3 + 2] * dx[5]);
            if (!(finite32(nq[0]) && finite32(nq[1]) && finite32(nq[2]) && finite32(nq[3]) && finite32(np[0]) && finite32(np[1]) && finite32(np[2])))
                outcome = STEP_NOT_FINITE;
        }
        if (trace) trace[TR_STEP0 + step] = outcome;
        if (outcome != STEP_TAKEN) break;
        memcpy(ps, nq, sizeof(nq));
        memcpy(ps + 4, np, sizeof(np));
        if (trace) ++trace[TR_STEPS];
    }
    /* 6. the end: w >= 0, the statuses */
    if (ok) {
        const int negated = ps[0] < 0.0f;
        if (negated) ps[0] = -ps[0], ps[1] = -ps[1], ps[2] = -ps[2], ps[3] = -ps[3];
        if (trace) trace[TR_FINAL_NEGATED] = negated;
        float R[9];
        rotation_of(ps, R);
        int32_t kept = 0;
        for (int32_t j = 0; j < m; ++j) {
            float c[3];
            camera_of(R, ps + 4, part + j, c);
            if (inlier(c[0], c[1], c[2], part[j].x, part[j].y, ry, tn2)) {
                ++kept;
            } else {
                status[list[j]] = LARGE_RESIDUAL;
            }
        }
        memcpy(pose, ps, sizeof(ps));
        n_inliers[0] = kept, best_out[0] = best, valid[0] = 1;
    }
    free(part), free(list), free(counts), free(models), free(tree);
    return 0;
}
