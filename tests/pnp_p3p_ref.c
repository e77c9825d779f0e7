/* pnp_p3p_ref.c — the scalar CPU restatement of PnpRansac's "p3p" sampler: hypotheses from three participants by
 * Grunert's quartic, the fourth participant choosing among the solutions; the scan, the score, select, the refit and finish are pnp_ref.c's
 * statements (included below and not edited: its static helpers are called with its CONTRACT variant).
 *
 * TEST INFRASTRUCTURE ONLY.  Every float operation of the contract in the order DESIGN.md 5.30a states it, float32, compiled without
 * contraction (tests/ref_build.py's STRICT flags); `/` and sqrtf are correctly rounded; no other libm call.  The device
 * (csrc/pnp_kernels.hip, pnp_p3p_hypothesis_kernel) is held to this file bit for bit by tests/test_pnp_p3p_gpu.py;
 * tests/test_pnp_p3p_cpu.py pins this file to tests/pnp_p3p_ref64.py and to ground truth.  `variant` 0 is the contract; the others are the
 * mutants that the CPU tests must catch.
 */
#include "pnp_ref.c"

enum { P3P_SAMPLE = 4, P3P_REFIT_MIN = 6, P3P_CUBIC_STEPS = 64, P3P_CUBIC_POLISH = 4, P3P_NEWTON_STEPS = 1 };
#define P3P_RESIDUAL 0.0000152587890625f /* 2^-16 */
enum { P3P_CONTRACT = 0, P3P_FOURTH_IGNORED = 1, P3P_FRONT_NOT_TESTED = 2, P3P_TIE_TAKES_LAST = 3, P3P_Y_UNSCALED = 4, P3P_ONE_NEWTON_STEP_FEWER = 5 };

/* What the three participants fix before any root is known. */
typedef struct {
    float f[3][3];          /* the unit bearings */
    float c01, c02, c12;    /* their cosines */
    float d01[3], d02[3];   /* X1 - X0, X2 - X0 */
    float n[3], nn;         /* d01 x d02 and its squared length */
    float a, b, c;          /* |X2 - X1|^2, |X2 - X0|^2, |X1 - X0|^2 */
    float N[3], D[2];       /* u = N(w) / D(w), lowest power first */
    float alpha2;           /* 2 (1 - c02) */
    float v[4];             /* the real roots w = s2 / s0 - 1 in the order they are produced */
    int roots;
} P3p;

static void cross3(const float *p, const float *q, float *r) {
    r[0] = p[1] * q[2] - p[2] * q[1];
    r[1] = p[2] * q[0] - p[0] * q[2];
    r[2] = p[0] * q[1] - p[1] * q[0];
}

static float dot3(const float *p, const float *q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }

/* The real roots of x^2 + beta x + gamma, the one with + sqrt first. */
static void p3p_quadratic(float beta, float gamma, float *v, int *roots) {
    const float disc = beta * beta - 4.0f * gamma;
    if (disc >= 0.0f) {
        const float sq = sqrtf(disc);
        v[(*roots)++] = (-beta + sq) * 0.5f;
        v[(*roots)++] = (-beta - sq) * 0.5f;
    }
}

/* One Newton step on y^3 + r2 y^2 + r1 y + r0; a step that is not finite is not taken. */
static float p3p_cubic_step(float y, float r2, float r1, float r0) {
    const float val = ((y + r2) * y + r1) * y + r0;
    const float der = (3.0f * y + 2.0f * r2) * y + r1;
    const float step = val / der;
    return finite32(step) ? y - step : y;
}

/* 0: the degeneracy test fired (two equal bearings, coincident or collinear landmarks, anything not finite). */
static int p3p_setup(const Part *q[3], P3p *s) {
    for (int k = 0; k < 3; ++k) {
        const float len = sqrtf((q[k]->x * q[k]->x + q[k]->y * q[k]->y) + 1.0f);
        s->f[k][0] = q[k]->x / len, s->f[k][1] = q[k]->y / len, s->f[k][2] = 1.0f / len;
    }
    s->c01 = dot3(s->f[0], s->f[1]), s->c02 = dot3(s->f[0], s->f[2]), s->c12 = dot3(s->f[1], s->f[2]);
    float g1[3], g2[3], m[3], d12[3];
    for (int e = 0; e < 3; ++e) g1[e] = s->f[1][e] - s->f[0][e], g2[e] = s->f[2][e] - s->f[0][e];
    cross3(g1, g2, m);
    const float mm = dot3(m, m);
    if (!(finite32(mm) && mm > 0.0f)) return 0;
    s->d01[0] = q[1]->X - q[0]->X, s->d01[1] = q[1]->Y - q[0]->Y, s->d01[2] = q[1]->Z - q[0]->Z;
    s->d02[0] = q[2]->X - q[0]->X, s->d02[1] = q[2]->Y - q[0]->Y, s->d02[2] = q[2]->Z - q[0]->Z;
    d12[0] = q[2]->X - q[1]->X, d12[1] = q[2]->Y - q[1]->Y, d12[2] = q[2]->Z - q[1]->Z;
    s->c = dot3(s->d01, s->d01), s->b = dot3(s->d02, s->d02), s->a = dot3(d12, d12);
    cross3(s->d01, s->d02, s->n);
    s->nn = dot3(s->n, s->n);
    if (!(finite32(s->nn) && s->nn > 0.0f)) return 0;
    /* with s1 = u s0, s2 = v s0 and v = 1 + w (the depths of a sample are alike, so the roots in v crowd about 1; in w they stand apart):
     * u = N(w) / D(w) from the difference of the two ratio equations, then the quartic in w.  The small terms come from differences of
     * bearings, not of cosines: alpha = 1 - c02 = |f2 - f0|^2 / 2, delta = c12 - c01 = f1 . (f2 - f0). */
    const float alpha = 0.5f * dot3(g2, g2), delta = dot3(s->f[1], g2);
    const float B = s->a / s->b, k = (s->c - s->a) / s->b;
    const float n0 = 2.0f * (k * alpha), n1 = n0 + 2.0f, n2 = k + 1.0f;
    const float e0 = 2.0f * delta, e1 = 2.0f * s->c12;
    s->N[0] = n0, s->N[1] = n1, s->N[2] = n2, s->D[0] = e0, s->D[1] = e1, s->alpha2 = 2.0f * alpha;
    const float a2 = s->alpha2, t12 = 2.0f * s->c12;
    const float g0 = e0 * e0, g1c = 2.0f * (e0 * e1), g2c = e1 * e1;                         /* D^2 */
    const float h0 = n0 * e0, h1 = n0 * e1 + n1 * e0, h2 = n1 * e1 + n2 * e0, h3 = n2 * e1;  /* N D */
    /* N^2 + (1 + w)^2 D^2 - 2 c12 (1 + w) N D - B (2 alpha + 2 alpha w + w^2) D^2, each power's four terms in this order */
    const float k4 = ((n2 * n2 + g2c) - t12 * h3) - B * g2c;
    const float k3 = ((2.0f * (n1 * n2) + (2.0f * g2c + g1c)) - t12 * (h3 + h2)) - B * (a2 * g2c + g1c);
    const float k2 = (((2.0f * (n0 * n2) + n1 * n1) + ((g2c + 2.0f * g1c) + g0)) - t12 * (h2 + h1)) - B * ((a2 * g2c + a2 * g1c) + g0);
    const float k1 = ((2.0f * (n0 * n1) + (g1c + 2.0f * g0)) - t12 * (h1 + h0)) - B * (a2 * g1c + a2 * g0);
    const float k0 = ((n0 * n0 + g0) - t12 * h0) - B * (a2 * g0);
    if (!(finite32(k4) && k4 != 0.0f)) return 0;
    const float p3 = k3 / k4, p2 = k2 / k4, p1 = k1 / k4, p0 = k0 / k4;
    /* Ferrari: the largest real root y of the resolvent cubic by Newton from Cauchy's bound, a fixed number of steps */
    const float r2 = -p2, r1 = p3 * p1 - 4.0f * p0, r0 = (4.0f * (p2 * p0) - (p3 * p3) * p0) - p1 * p1;
    float bound = fabsf(r2);
    if (fabsf(r1) > bound) bound = fabsf(r1);
    if (fabsf(r0) > bound) bound = fabsf(r0);
    /* Newton from Cauchy's bound on the side of the inflection point xi where the cubic keeps one sign of curvature up to its outermost
     * root: from above when the cubic is <= 0 at xi (the largest root lies above xi), from below otherwise (the smallest lies below) */
    const float xi = -r2 / 3.0f;
    const float at_xi = ((xi + r2) * xi + r1) * xi + r0;
    float y = at_xi > 0.0f ? -(1.0f + bound) : 1.0f + bound;
    for (int i = 0; i < P3P_CUBIC_STEPS; ++i) y = p3p_cubic_step(y, r2, r1, r0);
    /* the other two roots by deflation; the largest real root of the three, then polished on the cubic itself */
    const float db = r2 + y, dc = r1 + db * y;
    const float ddisc = db * db - 4.0f * dc;
    if (ddisc >= 0.0f) {
        const float other = (-db + sqrtf(ddisc)) * 0.5f;
        if (other > y) y = other;
    }
    for (int i = 0; i < P3P_CUBIC_POLISH; ++i) y = p3p_cubic_step(y, r2, r1, r0);
    /* x^4 + p3 x^3 + p2 x^2 + p1 x + p0 = (x^2 + p3/2 x + y/2)^2 - (R x + S)^2; the larger of R^2, S^2 takes the square root */
    const float hp = 0.5f * p3, hy = 0.5f * y;
    const float R2 = (hp * hp - p2) + y, S2 = hy * hy - p0, RS = 0.5f * (hp * y - p1);
    float R = 0.0f, S = 0.0f;
    if (R2 >= S2 && R2 > 0.0f) {
        R = sqrtf(R2), S = RS / R;
    } else if (S2 > 0.0f) {
        S = sqrtf(S2), R = RS / S;
    }
    s->roots = 0;
    p3p_quadratic(hp + R, hy + S, s->v, &s->roots);
    p3p_quadratic(hp - R, hy - S, s->v, &s->roots);
    return 1;
}

/* The pose [R | t] of root w: the distances, their Newton steps, the two frames.  0: a distance is not positive or an entry is not finite. */
static int p3p_pose(const Part *q[3], const P3p *s, float w, int variant, float *P) {
    const float u = ((s->N[2] * w + s->N[1]) * w + s->N[0]) / (s->D[1] * w + s->D[0]);
    const float v = 1.0f + w;
    const float qv = (w * w + s->alpha2 * w) + s->alpha2;
    float s0 = sqrtf(s->b / qv), s1 = u * s0, s2 = v * s0;
    const int steps = variant == P3P_ONE_NEWTON_STEP_FEWER ? P3P_NEWTON_STEPS - 1 : P3P_NEWTON_STEPS;
    for (int i = 0; i < steps; ++i) { /* Newton on the three distance equations, Cramer's rule */
        const float q0 = ((s0 * s0 + s1 * s1) - (2.0f * s->c01) * (s0 * s1)) - s->c;
        const float q1 = ((s0 * s0 + s2 * s2) - (2.0f * s->c02) * (s0 * s2)) - s->b;
        const float q2 = ((s1 * s1 + s2 * s2) - (2.0f * s->c12) * (s1 * s2)) - s->a;
        const float j00 = 2.0f * (s0 - s1 * s->c01), j01 = 2.0f * (s1 - s0 * s->c01);
        const float j10 = 2.0f * (s0 - s2 * s->c02), j12 = 2.0f * (s2 - s0 * s->c02);
        const float j21 = 2.0f * (s1 - s2 * s->c12), j22 = 2.0f * (s2 - s1 * s->c12);
        const float det = -(j00 * (j12 * j21)) - j01 * (j10 * j22);
        const float m12 = q1 * j22 - j12 * q2;
        const float x0 = (-(q0 * (j12 * j21)) - j01 * m12) / det;
        const float x1 = (j00 * m12 - q0 * (j10 * j22)) / det;
        const float x2 = ((-(j00 * (q1 * j21)) - j01 * (j10 * q2)) + q0 * (j10 * j21)) / det;
        s0 = s0 - x0, s1 = s1 - x1, s2 = s2 - x2;
    }
    if (!(s0 > 0.0f && s1 > 0.0f && s2 > 0.0f)) return 0;
    { /* a root the steps did not bring onto the three equations is no solution: each residual within 2^-16 of its two squares' sum */
        const float t0 = s0 * s0, t1 = s1 * s1, t2 = s2 * s2;
        const float q0 = ((t0 + t1) - (2.0f * s->c01) * (s0 * s1)) - s->c;
        const float q1 = ((t0 + t2) - (2.0f * s->c02) * (s0 * s2)) - s->b;
        const float q2 = ((t1 + t2) - (2.0f * s->c12) * (s1 * s2)) - s->a;
        if (!(fabsf(q0) <= P3P_RESIDUAL * (t0 + t1) && fabsf(q1) <= P3P_RESIDUAL * (t0 + t2) && fabsf(q2) <= P3P_RESIDUAL * (t1 + t2))) return 0;
    }
    float Y0[3], e1[3], e2[3], e3[3], i1[3], i2[3];
    for (int e = 0; e < 3; ++e) {
        Y0[e] = s0 * s->f[0][e];
        e1[e] = s1 * s->f[1][e] - Y0[e];
        e2[e] = s2 * s->f[2][e] - Y0[e];
    }
    cross3(e1, e2, e3);
    cross3(s->d02, s->n, i1);
    cross3(s->n, s->d01, i2);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) P[r * 4 + c] = ((e1[r] * i1[c] + e2[r] * i2[c]) + e3[r] * s->n[c]) / s->nn;
        P[r * 4 + 3] = Y0[r] - ((P[r * 4] * q[0]->X + P[r * 4 + 1] * q[0]->Y) + P[r * 4 + 2] * q[0]->Z);
    }
    for (int i = 0; i < 12; ++i) {
        if (!finite32(P[i])) return 0;
    }
    return 1;
}

/* Whether a solution with error `err` replaces the best so far. */
static int p3p_better(float err, float best, int have, int variant) {
    if (!have) return 1;
    return variant == P3P_TIE_TAKES_LAST ? err <= best : err < best;
}

/* The choice among n candidates' errors alone (the tests drive it at a tie): the index of the winner, -1: none. */
int p3p_choose(const float *err, int32_t n, int32_t variant) {
    int best = -1;
    for (int i = 0; i < n; ++i) {
        if (p3p_better(err[i], best < 0 ? 0.0f : err[best], best >= 0, variant)) best = i;
    }
    return best;
}

/* The solver alone: xy [3][2] calibrated pixels, X [3][3] landmarks -> the solutions [4][12] in the order they are produced; their number,
 * -1: the degeneracy test fired. */
int p3p_solve(const float *xy, const float *X, int32_t variant, float *sols) {
    Part part[3];
    const Part *q[3];
    for (int k = 0; k < 3; ++k) {
        part[k].x = xy[2 * k], part[k].y = xy[2 * k + 1], part[k].X = X[3 * k], part[k].Y = X[3 * k + 1], part[k].Z = X[3 * k + 2];
        q[k] = part + k;
    }
    P3p s;
    if (!p3p_setup(q, &s)) return -1;
    int count = 0;
    for (int i = 0; i < s.roots; ++i) count += p3p_pose(q, &s, s.v[i], variant, sols + 12 * count);
    return count;
}

/* One hypothesis: [R | t] of four participants, 0 = invalid.  solutions (may be NULL): how many the solver returned, -1: degenerate. */
static int p3p_fit(const Part *q[P3P_SAMPLE], float ry, int variant, float *P, int32_t *solutions) {
    P3p s;
    if (solutions) *solutions = -1;
    if (!p3p_setup(q, &s)) return 0;
    int have = 0, count = 0;
    float best = 0.0f;
    for (int i = 0; i < s.roots; ++i) {
        float Q[12], c[3];
        if (!p3p_pose(q, &s, s.v[i], variant, Q)) continue;
        ++count;
        int front = 1;
        for (int k = 0; k < P3P_SAMPLE; ++k) {
            project(Q, q[k], c);
            front = front && c[2] > 0.0f;
        }
        if (!front && variant != P3P_FRONT_NOT_TESTED) continue;
        const float ex = c[0] - q[3]->x * c[2];
        const float ey = (c[1] - q[3]->y * c[2]) * (variant == P3P_Y_UNSCALED ? 1.0f : ry);
        const float err = ex * ex + ey * ey;
        if (!finite32(err)) continue;
        if (variant == P3P_FOURTH_IGNORED ? !have : p3p_better(err, best, have, variant)) {
            memcpy(P, Q, sizeof(Q));
            best = err, have = 1;
        }
    }
    if (solutions) *solutions = count;
    return have;
}

/* One hypothesis from four rows of (x, y, X, Y, Z), for the tests of samples. */
int p3p_hypothesis(const float *rows, float ry, int32_t variant, float *P, int32_t *solutions) {
    Part part[P3P_SAMPLE];
    const Part *q[P3P_SAMPLE];
    for (int k = 0; k < P3P_SAMPLE; ++k) {
        part[k].x = rows[5 * k], part[k].y = rows[5 * k + 1], part[k].X = rows[5 * k + 2], part[k].Y = rows[5 * k + 3], part[k].Z = rows[5 * k + 4];
        q[k] = part + k;
    }
    const int ok = p3p_fit(q, ry, variant, P, solutions);
    if (!ok) memset(P, 0, sizeof(float) * 12);
    return ok;
}

/* pnp_solve's arguments; solutions [hypotheses] (may be NULL): the solver's count per hypothesis, -1: no draw or degenerate. */
int pnp_p3p_solve(const float *landmarks, const float *uv, uint8_t *status, int32_t n, const float *K4, float threshold, int32_t hypotheses,
                  uint32_t seed, int32_t refine, int32_t variant, float *pose, int32_t *n_inliers, int32_t *best_out, int32_t *valid,
                  int32_t *counts_out, float *models_out, float *sums27, int32_t *trace, int32_t *solutions) {
    if (n < 1 || n > 65536 || hypotheses < 1 || hypotheses > 4096 || refine < 0 || refine > MAX_STEPS) return -1;
    const float fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    const float tn = threshold / fx, tn2 = tn * tn;
    const float ry = fy / fx;
    Part *part = malloc(sizeof(Part) * (size_t)n);
    int32_t *list = malloc(sizeof(int32_t) * (size_t)n);
    int32_t *counts = malloc(sizeof(int32_t) * (size_t)hypotheses);
    float *models = malloc(sizeof(float) * 12 * (size_t)hypotheses);
    float(*tree)[TILE] = malloc(sizeof(float) * SUMS * TILE);
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
        if (X == 0.0f && Y == 0.0f && Z == 0.0f) continue;
        part[m].x = (u - cx) / fx, part[m].y = (v - cy) / fy, part[m].X = X, part[m].Y = Y, part[m].Z = Z;
        list[m++] = i;
    }
    /* 2., 3. the hypotheses and their counts; 4. the winner: the highest count, the lowest index among equals */
    int32_t best = -1, best_count = -1;
    for (int32_t h = 0; h < hypotheses; ++h) {
        uint32_t idx[P3P_SAMPLE];
        int ok = m >= P3P_SAMPLE;
        for (int k = 0; k < P3P_SAMPLE; ++k) {
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
        if (solutions) solutions[h] = -1;
        if (ok) {
            const Part *q[P3P_SAMPLE];
            for (int k = 0; k < P3P_SAMPLE; ++k) q[k] = part + idx[k];
            ok = p3p_fit(q, ry, variant, P, solutions ? solutions + h : NULL);
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
    int ok = best >= 0 && pose_of_model(models + 12 * (size_t)(best < 0 ? 0 : best), CONTRACT, ps, trace);
    if (ok && trace) trace[TR_WINNER] = best, trace[TR_STEPS] = 0;
    /* 5. the refit: pnp_ref.c's, fewer than six rows end it */
    for (int step = 0; ok && step < refine; ++step) {
        float R[9], sums[SUMS], term[SUMS];
        rotation_of(ps, R);
        const float *first = step == 0 ? models + 12 * (size_t)best : NULL;
        int32_t count = 0;
        for (int e = 0; e < SUMS; ++e) sums[e] = 0.0f;
        for (int32_t base = 0; base < m; base += TILE) {
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
        if (step == 0 && sums27) memcpy(sums27, sums, sizeof(sums));
        int outcome = STEP_TAKEN;
        float dx[6], nq[4], np[3];
        if (count < P3P_REFIT_MIN) {
            outcome = STEP_FEW_INLIERS;
        } else if (!ldlt6(sums, dx)) {
            outcome = STEP_NOT_POSITIVE_DEFINITE;
        } else {
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
