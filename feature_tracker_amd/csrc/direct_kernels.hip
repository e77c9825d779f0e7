// direct_kernels.hip — DirectMethod (photometric 6-DoF pose alignment) on gfx950: SURVEY.md
// section 8(f) rank 4.  Replaces DirectMethod::TrackFeatures (camera-frame overload,
// src/direct_method_tracker/direct_method_tracker.cpp:35-86) with TrackAllFeaturesDirect (:115-192).
//
// The problem is ONE pose for all features: every Gauss-Newton iteration sums 21 + 6 normal-equation
// entries over features x patch pixels (50 700 terms for the reference's 300 features at 13 x 13),
// solves a 6 x 6 system and moves the pose.  Results must be those of the scalar loop, whose sums
// run feature by feature, pixel by pixel with one rounding per addition — and the convergence test
// (|dx|^2 < 1e-6) turns any reordering into a different iteration count.  So the kernel keeps the
// order and parallelises what the order leaves free:
//
//   * one workgroup of 8 wavefronts per pose problem (problems are independent: blockIdx.x);
//   * waves 1..7 are PRODUCERS: chunk c = 64 consecutive terms of the (feature, pixel) stream; a
//     lane projects its feature with the current pose, takes the six bounds-checked bilinear taps
//     (five in the current image, one in the reference image) straight from global memory, forms
//     the 1 x 6 Jacobian row and writes the 27 products of its pixel into a ring slot in LDS;
//   * wave 0 is the CONSUMER: lane k < 27 adds row k of every chunk in stream order (the exact-order
//     chain of the KLT kernels, klt_basic_kernels.hip);
//   * one barrier per round of 7 chunks; after the last round wave 0 solves the 6 x 6 system with
//     the lane-parallel Eigen-compatible LDLT (klt_ldlt.h: rows on lanes 0..5), publishes dx in
//     LDS, and every thread applies the same pose update, so the pose lives in registers.
//
// Projection of the features (cur_pixel_uv, :141-142) happens once per iteration in a prologue pass
// and is kept in LDS for the producers; the Jacobian of the pixel w.r.t. the pose (:145-148) depends
// on the reference-frame point only and is recomputed per lane (12 products).
// fp32 throughout, no contraction; quaternion arithmetic as defined in oracle/oracle_direct_method.c.
#define FTK_CHAIN_ROUND 8  // 32 terms per prefetch round (four: +2 % on the spread kernel, whose consumer does nothing but chain; the one-workgroup kernel does not care)
#include "klt_chain.h"
#include "klt_ldlt.h"
#include "match_plan.h"

namespace ftk {
namespace {

// In the ONE-workgroup kernel ten waves (nine producers), chain rounds of eight reads and a raised priority for the chain wave change
// nothing (3.56 / 3.49 / 3.47 ms against 3.49 for the 300-point problem): that kernel is bound by what one compute unit can issue per
// iteration (793 chunks x ~390 producer instructions + 50 700 x 1.4 chain instructions), not by the split of that work over its waves —
// which is why a single problem is SPREAD over the chip (direct_track_spread_kernel below: 2.53 ms); there the consumer only chains,
// and longer chain rounds and the raised priority pay (docs/LAB_NOTES.md).
constexpr int kDmProducers = kDmWaves - 1;
constexpr int kDmChunk = 64;
constexpr int kDmRow = kDmChunk + 4;  // row pitch in floats: keeps the consumer's b128 reads on distinct banks
constexpr int kDmTerms = 27;          // 21 upper-triangle H entries (row-major) + 6 b entries
constexpr float kZeroFloat = 1e-6f;

struct Quat {
    float x, y, z, w;
};

__device__ __forceinline__ Quat q_mul(const Quat &a, const Quat &b) {
    Quat r;
    r.x = (a.x * b.w - a.z * b.y) + (a.y * b.z + a.w * b.x);
    r.y = (a.y * b.w - a.x * b.z) + (a.z * b.x + a.w * b.y);
    r.z = (a.z * b.w - a.y * b.x) + (a.x * b.y + a.w * b.z);
    r.w = (a.w * b.w - a.x * b.x) - (a.z * b.z + a.y * b.y);
    return r;
}
__device__ __forceinline__ float q_squared_norm(const Quat &q) { return (q.x * q.x + q.z * q.z) + (q.y * q.y + q.w * q.w); }
__device__ __forceinline__ Quat q_inverse(const Quat &q) {
    const float n2 = q_squared_norm(q);
    Quat r = {0.0f, 0.0f, 0.0f, 0.0f};
    if (n2 > 0.0f) {
        r.x = -q.x / n2;
        r.y = -q.y / n2;
        r.z = -q.z / n2;
        r.w = q.w / n2;
    }
    return r;
}
__device__ __forceinline__ Quat q_normalized(Quat q) {
    const float z = q_squared_norm(q);
    if (z > 0.0f) {
        const float n = sqrtf(z);
        q.x /= n;
        q.y /= n;
        q.z /= n;
        q.w /= n;
    }
    return q;
}
__device__ __forceinline__ void q_rotate(const Quat &q, float vx, float vy, float vz, float &ox, float &oy, float &oz) {
    float ux = q.y * vz - q.z * vy, uy = q.z * vx - q.x * vz, uz = q.x * vy - q.y * vx;
    ux += ux;
    uy += uy;
    uz += uz;
    const float cx = q.y * uz - q.z * uy, cy = q.z * ux - q.x * uz, cz = q.x * uy - q.y * ux;
    ox = (vx + q.w * ux) + cx;
    oy = (vy + q.w * uy) + cy;
    oz = (vz + q.w * uz) + cz;
}

// GrayImage::GetPixelValue straight from global memory (no LDS window: every tap of a problem is touched once per iteration,
// and the images stay in L2), in two halves so that the SIX taps of a term have all their 24 byte loads in flight before the
// first value is formed: the producers were bound by six dependent round trips per term (sample() returns early on an invalid
// coordinate, and the compiler keeps the taps behind one another).  An invalid tap reads pixel (0, 0) and is not used.  Same
// validity rule, fractions, weight products and sum order as sample() (klt_window.h).
struct DmTap {
    bool valid;
    float w_tl, w_tr, w_bl, w_br;
    uint8_t p00, p01, p10, p11;
};

__device__ __forceinline__ void dm_tap_issue(DmTap &t, const DevImage &im, float row, float col) {
    t.valid = row >= 0.0f && col >= 0.0f && row <= (float)(im.rows - 1) && col <= (float)(im.cols - 1);
    const float r = t.valid ? row : 0.0f, c = t.valid ? col : 0.0f;
    const int r0 = (int)r, c0 = (int)c;
    const float sub_row = __builtin_amdgcn_fractf(r), sub_col = __builtin_amdgcn_fractf(c);
    const float inv_sub_row = 1.0f - sub_row, inv_sub_col = 1.0f - sub_col;
    t.w_tl = inv_sub_row * inv_sub_col;
    t.w_tr = inv_sub_row * sub_col;
    t.w_bl = sub_row * inv_sub_col;
    t.w_br = sub_row * sub_col;
    const int r1 = (r0 + 1 < im.rows) ? r0 + 1 : r0, c1 = (c0 + 1 < im.cols) ? c0 + 1 : c0;
    const unsigned top = __umul24((unsigned)r0, (unsigned)im.cols), bottom = __umul24((unsigned)r1, (unsigned)im.cols);
    t.p00 = im.data[top + (unsigned)c0];
    t.p01 = im.data[top + (unsigned)c1];
    t.p10 = im.data[bottom + (unsigned)c0];
    t.p11 = im.data[bottom + (unsigned)c1];
}

__device__ __forceinline__ float dm_tap_value(const DmTap &t) {
    return t.w_tl * (float)t.p00 + t.w_tr * (float)t.p01 + t.w_bl * (float)t.p10 + t.w_br * (float)t.p11;
}

__device__ __forceinline__ float dm_chain_chunk(float acc, const float *row) {
    const float4 *t = reinterpret_cast<const float4 *>(row);
    float4 qa[kChainRound], qb[kChainRound];
    chain_load(qa, t);
#pragma unroll
    for (int i = 0; i < kDmChunk / 4; i += 2 * kChainRound) {
        chain_load(qb, t + i + kChainRound);
        acc = chain_consume_all(acc, qa);
        if (i + 2 * kChainRound < kDmChunk / 4) {
            chain_load(qa, t + i + 2 * kChainRound);
        }
        acc = chain_consume_all(acc, qb);
    }
    return acc;
}

// The spread kernel's chain: a QUAD of lanes per sum (klt_chain.h, chain_quad_step16 — the same left-to-right sum, 16 terms per
// ds_read_b128 and 4.84 cycles per term instead of one lane's ~7).  `t`: this lane's first float4 of the round's first chunk (row of
// its sum, floats 4 (lane & 3) ..); a chunk's 64 terms are four steps of 16, the chunks of a round lie kDmTerms rows apart.  The
// reads of chunk w + 1 are issued before chunk w's 64 adds; with kChunks a constant the loop unrolls and every address is an
// immediate offset of one base register (6 chunks x 7 344 B < 64 KB).
constexpr int kDmChunkStep4 = kDmTerms * kDmRow / 4;  // float4 from one chunk of the ring to the next
__device__ __forceinline__ void dm_quad_reads(float4 (&a)[4], const float4 *t) {
    a[0] = t[0];
    a[1] = t[4];
    a[2] = t[8];
    a[3] = t[12];
}
__device__ __forceinline__ float dm_quad_adds(float acc, const float4 (&a)[4]) { return chain_quad_step64(acc, a[0], a[1], a[2], a[3]); }
template <int kChunks>
__device__ __forceinline__ float dm_chain_quads_round(float acc, const float4 *t) {
    float4 a[4], b[4];
    dm_quad_reads(a, t);
#pragma unroll
    for (int w = 0; w < kChunks; w += 2) {
        if (w + 1 < kChunks) {
            dm_quad_reads(b, t + (w + 1) * kDmChunkStep4);
        }
        __builtin_amdgcn_sched_barrier(0);
        acc = dm_quad_adds(acc, a);
        if (w + 2 < kChunks) {
            dm_quad_reads(a, t + (w + 2) * kDmChunkStep4);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (w + 1 < kChunks) {
            acc = dm_quad_adds(acc, b);
        }
    }
    return acc;
}
// (the stream's last round: any number of chunks)
__device__ __forceinline__ float dm_chain_quads_tail(float acc, const float4 *t, int chunks) {
    float4 a[4];
#pragma nounroll
    for (int w = 0; w < chunks; ++w) {
        dm_quad_reads(a, t + w * kDmChunkStep4);
        __builtin_amdgcn_sched_barrier(0);
        acc = dm_quad_adds(acc, a);
    }
    return acc;
}

// ---- pieces shared by the one-workgroup kernel and the spread kernel (same arithmetic by construction) ----

// Per level: the part of feature i's terms that does not change with the pose -> feat[4 i].w, feat[4 i + 1 .. 3]
__device__ __forceinline__ void dm_level_row(float4 *feat, const DirectProblem &pr, int i, float scale, float up, float fx, float fy) {
    const float prx = pr.p_ref[3 * i], pry = pr.p_ref[3 * i + 1], prz = pr.p_ref[3 * i + 2];
    const float scaled_ru = (pr.ref_uv[2 * i] / scale) * up, scaled_rv = (pr.ref_uv[2 * i + 1] / scale) * up;
    const float zi = 1.0f / prz;
    const float z2i = zi * zi;
    // jacobian_pixel_xi, :145-148 — operator precedence as written (j01 = j10 = 0)
    const float j00 = fx * zi, j02 = -fx * prx * z2i, j03 = -fx * prx * pry * z2i, j04 = fx + fx * prx * prx * z2i, j05 = -fx * pry * zi;
    const float j11 = fy * zi, j12 = -fy * pry * z2i, j13 = -fy - fy * pry * pry * z2i, j14 = fy * prx * pry * z2i, j15 = fy * prx * zi;
    feat[4 * i].w = scaled_ru;
    feat[4 * i + 1] = make_float4(scaled_rv, j00, j02, j03);
    feat[4 * i + 2] = make_float4(j04, j05, j11, j12);
    feat[4 * i + 3] = make_float4(j13, j14, j15, 0.0f);
}

// Projection of feature i with the current pose (:128-142) -> feat[4 i].xyz; write_uv: also cur_pixel_uv (:141-142)
__device__ __forceinline__ void dm_project(float4 *feat, const DirectProblem &pr, int i, const Quat &q_inv, float px, float py, float pz, float fx, float fy,
                                           float cx, float cy, bool write_uv) {
    const float prx = pr.p_ref[3 * i], pry = pr.p_ref[3 * i + 1], prz = pr.p_ref[3 * i + 2];
    float cu = 0.0f, cv = 0.0f;
    bool usable = !(prz < kZeroFloat);
    if (usable) {
        float cxp, cyp, czp;
        q_rotate(q_inv, prx - px, pry - py, prz - pz, cxp, cyp, czp);
        usable = !(czp < kZeroFloat);
        if (usable) {
            const float nx = cxp / czp, ny = cyp / czp;
            cu = fx * nx + cx;
            cv = fy * ny + cy;
            if (write_uv) {
                pr.cur_uv[2 * i] = cu;
                pr.cur_uv[2 * i + 1] = cv;
            }
        }
    }
    feat[4 * i].x = cu;
    feat[4 * i].y = cv;
    feat[4 * i].z = usable ? 1.0f : 0.0f;
}

// The 1 x 6 Jacobian row and the residual of one term of the (feature, pixel) stream (:144-168); in_range: the term exists
__device__ __forceinline__ void dm_term(const float4 *feat, const DirectParams &pp, const DevImage &ref, const DevImage &cur, bool in_range, int i, int pix,
                                        float inv_patch_cols, float (&jac)[6], float &residual) {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        jac[r] = 0.0f;
    }
    residual = 0.0f;
    if (in_range) {
        int prow = (int)((float)pix * inv_patch_cols);  // pix < 2^22: off by at most one, put right by the remainder
        int pcol = pix - prow * pp.patch_cols;
        if (pcol < 0) {
            --prow;
            pcol += pp.patch_cols;
        } else if (pcol >= pp.patch_cols) {
            ++prow;
            pcol -= pp.patch_cols;
        }
        const float4 f = feat[4 * i];
        if (f.z != 0.0f) {
            const float4 f1 = feat[4 * i + 1], f2 = feat[4 * i + 2], f3 = feat[4 * i + 3];
            const float drow = (float)(prow - pp.half_rows), dcol = (float)(pcol - pp.half_cols);
            const float row_i = drow + f1.x, col_i = dcol + f.w;
            const float row_j = drow + f.y, col_j = dcol + f.x;
            // all six must be valid (:160-162); evaluation order does not matter for the result
            DmTap a0, a1, a2, a3, a4, a5;
            dm_tap_issue(a0, cur, row_j, col_j - 1.0f);
            dm_tap_issue(a1, cur, row_j, col_j + 1.0f);
            dm_tap_issue(a2, cur, row_j - 1.0f, col_j);
            dm_tap_issue(a3, cur, row_j + 1.0f, col_j);
            dm_tap_issue(a4, ref, row_i, col_i);
            dm_tap_issue(a5, cur, row_j, col_j);
            const bool ok = a0.valid && a1.valid && a2.valid && a3.valid && a4.valid && a5.valid;
            const float t0 = dm_tap_value(a0), t1 = dm_tap_value(a1), t2 = dm_tap_value(a2), t3 = dm_tap_value(a3), t4 = dm_tap_value(a4),
                        t5 = dm_tap_value(a5);
            if (ok) {
                const float j00 = f1.y, j01 = 0.0f, j02 = f1.z, j03 = f1.w, j04 = f2.x, j05 = f2.y;
                const float j10 = 0.0f, j11 = f2.z, j12 = f2.w, j13 = f3.x, j14 = f3.y, j15 = f3.z;
                const float gx = (t1 - t0) * 0.5f, gy = (t3 - t2) * 0.5f;
                residual = t5 - t4;
                jac[0] = gx * j00 + gy * j10;
                jac[1] = gx * j01 + gy * j11;
                jac[2] = gx * j02 + gy * j12;
                jac[3] = gx * j03 + gy * j13;
                jac[4] = gx * j04 + gy * j14;
                jac[5] = gx * j05 + gy * j15;
            }
        }
    }
}

// wave 0: the 27 sums (lane k < 27 holds sum k) -> full symmetric H in LDS -> lane-parallel LDLT (klt_ldlt.h) -> dx at sums[68..74)
// (kPublish = false: the sums already lie in sums[0 .. 27), written behind a barrier by the waves that chained them)
template <bool kPublish = true>
__device__ __forceinline__ void dm_solve(float *sums, float acc, int lane) {
    if (kPublish && lane < kDmTerms) {
        sums[lane] = acc;
    }
    __builtin_amdgcn_wave_barrier();  // same-wave LDS traffic is ordered
    if (lane < 36) {
        const int r0 = lane / 6, c0 = lane - 6 * r0;
        const int r = r0 < c0 ? r0 : c0, cc = r0 < c0 ? c0 : r0;
        sums[32 + lane] = sums[r * (13 - r) / 2 + (cc - r)];  // upper triangle, row-major
    }
    __builtin_amdgcn_wave_barrier();
    const Ldlt6 fac = ldlt6_factor(sums + 32, lane);
    ldlt6_solve(fac, sums + 21, sums + 68, lane);
}

// The pose update (:170-181), redundantly in every thread; returns whether the level's iterations stop
__device__ __forceinline__ bool dm_update_pose(const float *sums, float converge, Quat &q, float &px, float &py, float &pz) {
    float dx[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        dx[k] = sums[68 + k];
    }
    bool has_nan = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        has_nan = has_nan || isnan(dx[k]);
    }
    if (has_nan) {
        return true;  // :173
    }
    px += dx[0];
    py += dx[1];
    pz += dx[2];
    Quat dq = {dx[3] * 0.5f, dx[4] * 0.5f, dx[5] * 0.5f, 1.0f};
    q = q_normalized(q_mul(q_normalized(dq), q));
    const float sq = (((dx[0] * dx[0] + dx[2] * dx[2]) + (dx[1] * dx[1] + dx[3] * dx[3])) + dx[4] * dx[4]) + dx[5] * dx[5];
    return sq < converge;  // :181
}

// TREE: the throughput mode (ftk_set_reduction_mode) — all eight waves sample, every lane keeps 27 partial sums, a butterfly and a
// fixed-order sum over the waves replace the ring and wave 0's exact-order chains (50 700 dependent adds per iteration at the
// reference's 300 points x 13 x 13).  Same products, another summation order: NOT bit-identical to the scalar loop; reported only.
template <bool TREE>
__global__ void __launch_bounds__(kDmWaves * kWave) direct_track_kernel(const DirectParams pp) {
    extern __shared__ float4 dm_lds[];
    const DirectProblem pr = pp.problems[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const bool consumer = wave == 0;
    float *const ring = reinterpret_cast<float *>(dm_lds);                   // [2][kDmProducers][kDmTerms][kDmRow]
    float *const sums = ring + 2 * kDmProducers * kDmTerms * kDmRow;         // [96]: 27 sums | H 6x6 at 32 | dx at 68
    // [n_track][4] float4: {cur u, cur v, usable, scaled ref u} (every iteration) | {scaled ref v, j00, j02, j03} | {j04, j05, j11, j12} |
    // {j13, j14, j15, -} (once per level: the reference position at this level and the non-trivial entries of jacobian_pixel_xi,
    // :145-148, which depend on the reference-frame point and the level's intrinsics only); in LDS, or in device memory for
    // problems too large for it (written and read by this workgroup only, with a workgroup barrier in between)
    float4 *const feat = pr.feat != nullptr ? pr.feat : reinterpret_cast<float4 *>(sums + 96);
    const int n = pr.n;
    const int n_track = (int)((uint32_t)n < pp.max_track_points ? (uint32_t)n : pp.max_track_points);
    const int P = pp.patch_rows * pp.patch_cols;
    const long long total_terms = (long long)n_track * P;
    const int n_chunks = (int)((total_terms + kDmChunk - 1) / kDmChunk);
    const int n_rounds = (n_chunks + kDmProducers - 1) / kDmProducers;
    // Walking the (feature, pixel) stream without a division per term: a wave's first chunk gives its lane's (feature, pixel) once,
    // every further chunk is a constant number of terms on (all waves sample: kDmWaves chunks; the producers: kDmProducers) =
    // step_i features and step_pix pixels, with one carry.
    const int step_all_i = (kDmWaves * kDmChunk) / P, step_all_pix = (kDmWaves * kDmChunk) % P;
    const int step_prod_i = (kDmProducers * kDmChunk) / P, step_prod_pix = (kDmProducers * kDmChunk) % P;
    const float inv_patch_cols = 1.0f / (float)pp.patch_cols;
    auto term_start = [&](int first_chunk, int &i, int &pix) {
        const long long g = (long long)first_chunk * kDmChunk + lane;
        i = (int)(g / P);
        pix = (int)(g - (long long)i * P);
    };
    auto term_advance = [&](int &i, int &pix, int step_i, int step_pix) {
        i += step_i;
        pix += step_pix;
        if (pix >= P) {
            pix -= P;
            ++i;
        }
    };

    // pose in registers, identical in every thread
    Quat q = {pr.pose[1], pr.pose[2], pr.pose[3], pr.pose[0]};
    float px = pr.pose[4], py = pr.pose[5], pz = pr.pose[6];
    uint32_t iterations = 0;

    const float scale = (float)(1 << (pp.n_levels - 1));
    if (pp.method == FTK_METHOD_DIRECT && n_track > 0) {
        for (int level = pp.n_levels - 1; level > -1; --level) {
            const DevImage ref = pr.ref[level];
            const DevImage cur = pr.cur[level];
            // scaled_K / scaled_ref_points_: value / scale, then doubled once per finer level (exact), :47-52,64-69
            const float up = (float)(1 << (pp.n_levels - 1 - level));
            const float fx = (pr.K[0] / scale) * up, fy = (pr.K[1] / scale) * up, cx = (pr.K[2] / scale) * up, cy = (pr.K[3] / scale) * up;
            // ---- per level: the part of a term that does not change with the pose ----
            for (int i = tid; i < n_track; i += kDmWaves * kWave) {
                dm_level_row(feat, pr, i, scale, up, fx, fy);
            }
            bool stop = false;
            for (uint32_t iter = 0; iter < pp.max_iteration && !stop; ++iter) {
                ++iterations;
                // ---- projection of every feature with the current pose (:128-142) ----
                const Quat q_inv = q_inverse(q);
                for (int i = tid; i < n_track; i += kDmWaves * kWave) {
                    dm_project(feat, pr, i, q_inv, px, py, pz, fx, fy, cx, cy, true);
                }
                __syncthreads();

                // the 1 x 6 Jacobian row and the residual of term `lane` of a 64-term chunk of the (feature, pixel) stream (:144-168)
                // (i, pix): the feature and the patch pixel of this lane's term of `chunk` — kept by the caller, which walks its chunks
                // with a constant stride (term_advance below: no division per term; a 64-bit one cost more than the six taps)
                auto chunk_terms = [&](int chunk, int i, int pix, float (&jac)[6], float &residual) {
                    dm_term(feat, pp, ref, cur, chunk < n_chunks && i < n_track, i, pix, inv_patch_cols, jac, residual);
                };
                // ---- the (feature, pixel) stream in rounds of kDmProducers chunks ----
                float acc = 0.0f;
                if constexpr (TREE) {
                    float part[kDmTerms];
#pragma unroll
                    for (int k = 0; k < kDmTerms; ++k) {
                        part[k] = 0.0f;
                    }
                    int ti, tpix;
                    term_start(wave, ti, tpix);
                    for (int chunk = wave; chunk < n_chunks; chunk += kDmWaves) {
                        float jac[6], residual;
                        chunk_terms(chunk, ti, tpix, jac, residual);
                        term_advance(ti, tpix, step_all_i, step_all_pix);
                        int k = 0;
#pragma unroll
                        for (int r = 0; r < 6; ++r) {
#pragma unroll
                            for (int c = r; c < 6; ++c) {
                                part[k] += jac[r] * jac[c];
                                ++k;
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 6; ++r) {
                            part[21 + r] += residual * jac[r];
                        }
                    }
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
                        for (int k = 0; k < kDmTerms; ++k) {
                            part[k] += __shfl_xor(part[k], off, kWave);
                        }
                    }
                    float *const wave_sums = ring;  // unused in this mode: [wave][kDmTerms]
                    if (lane == 0) {
#pragma unroll
                        for (int k = 0; k < kDmTerms; ++k) {
                            wave_sums[wave * kDmTerms + k] = part[k];
                        }
                    }
                    __syncthreads();
                    if (consumer && lane < kDmTerms) {
                        acc = wave_sums[lane];
                        for (int w = 1; w < kDmWaves; ++w) {
                            acc += wave_sums[w * kDmTerms + lane];
                        }
                    }
                } else {
                int ti = 0, tpix = 0;
                if (!consumer) {
                    term_start(wave - 1, ti, tpix);
                }
                for (int round = 0; round < n_rounds; ++round) {
                    if (!consumer) {
                        const int chunk = round * kDmProducers + (wave - 1);
                        float *slot = ring + (((round & 1) * kDmProducers + (wave - 1)) * kDmTerms) * kDmRow;
                        float jac[6], residual;
                        chunk_terms(chunk, ti, tpix, jac, residual);
                        term_advance(ti, tpix, step_prod_i, step_prod_pix);
                        // an unused pixel contributes exact zeros (x + (+-0) == x, and the sums start at +0)
                        int k = 0;
#pragma unroll
                        for (int r = 0; r < 6; ++r) {
#pragma unroll
                            for (int c = r; c < 6; ++c) {
                                slot[k * kDmRow + lane] = jac[r] * jac[c];
                                ++k;
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 6; ++r) {
                            slot[(21 + r) * kDmRow + lane] = residual * jac[r];
                        }
                    }
                    __syncthreads();
                    if (consumer && lane < kDmTerms) {
                        for (int w = 0; w < kDmProducers; ++w) {
                            if (round * kDmProducers + w < n_chunks) {
                                acc = dm_chain_chunk(acc, ring + ((((round & 1) * kDmProducers + w) * kDmTerms) + lane) * kDmRow);
                            }
                        }
                    }
                }
                }
                if (consumer) {
                    dm_solve(sums, acc, lane);
                }
                __syncthreads();
                // ---- update, redundantly in every thread (:170-181) ----
                stop = dm_update_pose(sums, pp.converge, q, px, py, pz);
                __syncthreads();  // everyone has read `sums` and `feat` before the next iteration rewrites them
            }
        }
    }
    // ---- status and pose write-back (:72-83) ----
    const DevImage bottom = pr.ref[0];
    for (int i = tid; i < n; i += kDmWaves * kWave) {
        uint8_t s = pr.status_valid ? pr.status[i] : (uint8_t)FTK_TRACKED;
        const float u = pr.cur_uv[2 * i], v = pr.cur_uv[2 * i + 1];
        if (u < 0.0f || u > (float)(bottom.cols - 1) || v < 0.0f || v > (float)(bottom.rows - 1)) {
            s = FTK_OUTSIDE;
        }
        pr.status[i] = s;
    }
    if (tid == 0) {
        pr.pose[0] = q.w;
        pr.pose[1] = q.x;
        pr.pose[2] = q.y;
        pr.pose[3] = q.z;
        pr.pose[4] = px;
        pr.pose[5] = py;
        pr.pose[6] = pz;
        if (pr.iterations) {
            *pr.iterations = iterations;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// ONE pose problem spread over the chip (exact sums).  The one-workgroup kernel above is bound by what a single compute unit can
// issue per iteration — 793 chunks x ~390 producer instructions beside the 50 700-term chains (profiles/r4_pmc_direct.txt) — while
// 255 compute units idle.  Here workgroup 0 is the CONSUMER and keeps only the sequential part: six loader waves bring finished
// chunks from device memory into the LDS ring, waves 0 and 1 add them in stream order (a quad of lanes per sum: sums 0 .. 15 and
// 16 .. 26), wave 0 solves, everybody moves the pose.  Workgroups 1 .. NP are PRODUCERS: per iteration each takes the pose the
// consumer published, projects the features, and its waves form the terms of chunks w, w + 8 NP, ... (w = the wave's number over all
// producers: the first chunks of the stream come first).
// What crosses the chip per term is the 1 x 6 Jacobian row and the residual — 7 floats, not the 27 products: the loader wave that
// fetched them forms jac[r] * jac[c] and residual * jac[r] on its way into the ring, the same single-rounded fp32 products the
// one-workgroup kernel forms, so the sums see the same 27 x 64 rows (1 792 B per chunk through the consumer's memory queue
// instead of 6 912, a workspace of 1.4 MB instead of 5.5 MB at 300 points x 13 x 13, and a quarter of the producers' stores).
//
// Hand-offs (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement & inter-workgroup visibility"): every handed-off byte is stored
// AND loaded with agent-scope relaxed atomics (sc1: L2, never a stale L1 line); a storing wave waits for its stores (vmcnt(0))
// before one lane stores the flag; the wave that polled a flag is the wave that loads what it guards.
//   * consumer -> producers: pose[7] + level, then iter_tag = g + 1 (g counts iterations over all levels; 0xFFFFFFFF = leave);
//   * producer wave -> consumer loader wave: the chunk's 7 x 64 values (jac[0 .. 5], residual), then chunk_flag[c] = g + 1.
// A chunk slot is rewritten only after the consumer has published the NEXT pose, i.e. after it has consumed the whole stream.
// Every wait is BOUNDED (kSpreadMaxPolls): a wait that runs out poisons the pose with NaN and releases everybody — a bug or a
// launch that cannot become co-resident ends in a wrong answer the caller sees, never in a hung device.
// Results are those of the one-workgroup kernel bit for bit: same terms (dm_term), same order of the sums, same solve.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kSpreadStop = 0xFFFFFFFFu;
constexpr uint32_t kSpreadMaxPolls = 1u << 22;   // x (one L2 round trip + s_sleep) ~ seconds
constexpr int kSpreadHeaderWords = 64;           // iter_tag, error, level, -, pose[7] ...
constexpr int kSpreadValues = 7;                 // floats per term in the workspace: jac[0 .. 5], residual
constexpr int kSpreadChainWaves = 2;             // 27 sums x 4 lanes
constexpr int kSpreadLoaders = kDmWaves - kSpreadChainWaves;
static_assert(kSpreadLoaders <= kDmProducers, "the LDS ring is sized for the one-workgroup kernel's rounds");

__device__ __forceinline__ uint32_t spread_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void spread_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void spread_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// The flag itself.  Default: a relaxed sc1 store behind the storing wave's own `s_waitcnt vmcnt(0)` (every data store has been
// acknowledged by the memory side before the flag store is issued), and in the polling wave the guarded sc1 loads behind the branch
// on the polled value — MI355X_MICROARCH.md's second valid form for handed-off bytes that are ONLY ever touched by sc1 accesses: no
// cache holds a copy that could be stale, a wave issues its memory instructions in order and nothing is issued past an unresolved
// branch, and a compiler barrier on either side keeps the compiler from moving the accesses.  The alternative, an
// agent-scope RELEASE flag store and an agent-scope ACQUIRE fence behind the poll, gives the same results, but on gfx950 these are
// `buffer_wbl2 sc1` (a write-back of the XCD's L2) per produced chunk and `buffer_inv sc1` (an invalidate of it) per fetched chunk —
// 800 of each per iteration: the loader's seven loads then take 800 - 900 ns instead of 320, the consumer waits for its loaders,
// 1.32 -> 1.48 ms for one 300-point problem and 1.33 -> 1.72 ms for six side by side (profiles/r5_direct_spread_consumer.txt).
// tests/test_direct_method_gpu.py and the soak compare the spread kernel with the one-workgroup kernel.
__device__ __forceinline__ void spread_publish(uint32_t *p, uint32_t v) {
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    spread_store(p, v);
}
__device__ __forceinline__ void spread_acquired() {
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

// Polls *flag until it equals `want` (or `also`); false when the wait ran out.  Whole wave, uniform address.
__device__ __forceinline__ bool spread_wait(const uint32_t *flag, uint32_t want, uint32_t also, uint32_t &seen) {
    for (uint32_t polls = 0; polls < kSpreadMaxPolls; ++polls) {
        seen = spread_load(flag);
        if (seen == want || seen == also) {
            spread_acquired();
            return true;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    return false;
}

__global__ void __launch_bounds__(kDmWaves * kWave) direct_track_spread_kernel(const DirectParams pp) {
    extern __shared__ float4 dm_lds[];
    // a few problems side by side: 1 + pp.spread consecutive workgroups each, a workspace each
    const int group = 1 + pp.spread;
    const int problem = (int)blockIdx.x / group, role = (int)blockIdx.x - problem * group;
    const DirectProblem pr = pp.problems[problem];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int n = pr.n;
    const int n_track = (int)((uint32_t)n < pp.max_track_points ? (uint32_t)n : pp.max_track_points);
    const int P = pp.patch_rows * pp.patch_cols;
    const long long total_terms = (long long)n_track * P;
    const int n_chunks = (int)((total_terms + kDmChunk - 1) / kDmChunk);
    uint32_t *const header = pp.spread_ws + (size_t)problem * pp.spread_ws_words;
    uint32_t *const chunk_flag = header + kSpreadHeaderWords;
    uint32_t *const values = chunk_flag + ((n_chunks + 63) & ~63);  // [n_chunks][kSpreadValues][kDmChunk] floats (as bits)
    const float scale = (float)(1 << (pp.n_levels - 1));

    if (role == 0) {
        // ================= the consumer =================
        const bool chain_wave = wave < kSpreadChainWaves;
        if (chain_wave) {
            __builtin_amdgcn_s_setprio(3);  // the chain IS the launch: it goes ahead of the loader wave on its SIMD
        }
        float *const ring = reinterpret_cast<float *>(dm_lds);            // [2][kSpreadLoaders][kDmTerms][kDmRow] (of the [2][kDmProducers] allocated)
        float *const sums = ring + 2 * kDmProducers * kDmTerms * kDmRow;  // [96]
        const int n_rounds = (n_chunks + kSpreadLoaders - 1) / kSpreadLoaders;
        // chain waves: lanes 4 s .. 4 s + 3 of wave w hold sum 16 w + s (the lanes beyond sum 26 repeat it: DPP wants every lane on)
        const int my_sum = min(wave * 16 + (lane >> 2), kDmTerms - 1);
        const float4 *const my_terms = reinterpret_cast<const float4 *>(ring + my_sum * kDmRow) + (lane & 3);
        Quat q = {pr.pose[1], pr.pose[2], pr.pose[3], pr.pose[0]};
        float px = pr.pose[4], py = pr.pose[5], pz = pr.pose[6];
        uint32_t iterations = 0, g = 0;
        bool failed = pp.spread_poison != 0;
        if (tid == 0) {
            reinterpret_cast<uint32_t *>(sums)[80] = 0u;  // "a loader's wait ran out"
        }
        __syncthreads();
        for (int level = pp.n_levels - 1; level > -1 && !failed && n_track > 0; --level) {  // (a problem of a batch may be empty)
            bool stop = false;
            for (uint32_t iter = 0; iter < pp.max_iteration && !stop && !failed; ++iter) {
                ++iterations;
                // ---- publish the pose of iteration g ----
                if (tid == 0) {
                    spread_store(header + 2, (uint32_t)level);
                    spread_store(header + 4, __float_as_uint(q.x));
                    spread_store(header + 5, __float_as_uint(q.y));
                    spread_store(header + 6, __float_as_uint(q.z));
                    spread_store(header + 7, __float_as_uint(q.w));
                    spread_store(header + 8, __float_as_uint(px));
                    spread_store(header + 9, __float_as_uint(py));
                    spread_store(header + 10, __float_as_uint(pz));
                    spread_stores_done();
                    spread_publish(header, g + 1u);
                }
                // ---- the stream: the loaders bring round r + 1 into the ring while waves 0 and 1 add round r ----
                float acc = 0.0f;
                bool wait_failed = false;
                for (int round = 0; round < n_rounds; ++round) {
                    if (!chain_wave) {
                        const int chunk = round * kSpreadLoaders + (wave - kSpreadChainWaves);
                        if (chunk < n_chunks) {
                            uint32_t seen;
                            // (a wave whose wait has run out once does not wait again: the iteration is lost anyway, and a second
                            // full wait per remaining round would turn one bounded wait into minutes)
                            if (!wait_failed && !spread_wait(chunk_flag + chunk, g + 1u, g + 1u, seen)) {
                                wait_failed = true;
                            }
                            const uint32_t *src = values + (size_t)chunk * (kSpreadValues * kDmChunk) + lane;
                            float *slot = ring + (((round & 1) * kSpreadLoaders + (wave - kSpreadChainWaves)) * kDmTerms) * kDmRow + lane;
                            float jac[6];
#pragma unroll
                            for (int r = 0; r < 6; ++r) {
                                jac[r] = __uint_as_float(spread_load(src + r * kDmChunk));
                            }
                            const float residual = __uint_as_float(spread_load(src + 6 * kDmChunk));
                            // the 27 products of the term, as the one-workgroup kernel forms them (H upper triangle row-major, then b)
                            int k = 0;
#pragma unroll
                            for (int r = 0; r < 6; ++r) {
#pragma unroll
                                for (int c = r; c < 6; ++c) {
                                    slot[k * kDmRow] = jac[r] * jac[c];
                                    ++k;
                                }
                            }
#pragma unroll
                            for (int r = 0; r < 6; ++r) {
                                slot[(21 + r) * kDmRow] = residual * jac[r];
                            }
                        }
                    }
                    __syncthreads();
                    if (chain_wave) {
                        const float4 *t = my_terms + ((round & 1) * kSpreadLoaders) * kDmChunkStep4;
                        const int chunks = n_chunks - round * kSpreadLoaders;
                        acc = chunks >= kSpreadLoaders ? dm_chain_quads_round<kSpreadLoaders>(acc, t) : dm_chain_quads_tail(acc, t, chunks);
                    }
                }
                if (chain_wave && (lane & 3) == 0 && wave * 16 + (lane >> 2) < kDmTerms) {
                    sums[wave * 16 + (lane >> 2)] = acc;
                }
                __syncthreads();
                if (wave == 0) {
                    dm_solve<false>(sums, 0.0f, lane);
                }
                // a loader whose wait ran out: every thread learns it (the barrier below is the one the solve needs anyway)
                if (wait_failed && lane == 0) {
                    reinterpret_cast<uint32_t *>(sums)[80] = 1u;
                }
                __syncthreads();
                stop = dm_update_pose(sums, pp.converge, q, px, py, pz);
                failed = reinterpret_cast<const uint32_t *>(sums)[80] != 0u;
                __syncthreads();  // everyone has read `sums` before the next iteration rewrites them
                ++g;
            }
        }
        if (tid == 0) {
            if (failed) {
                spread_store(header + 1, 1u);
                q.x = q.y = q.z = q.w = px = py = pz = __uint_as_float(0x7FC00000u);
            }
            spread_publish(header, kSpreadStop);  // the producers leave
            pr.pose[0] = q.w;
            pr.pose[1] = q.x;
            pr.pose[2] = q.y;
            pr.pose[3] = q.z;
            pr.pose[4] = px;
            pr.pose[5] = py;
            pr.pose[6] = pz;
            if (pr.iterations) {
                *pr.iterations = iterations;
            }
        }
        return;
    }

    // ================= a producer =================
    const int np = pp.spread;
    const int producer = role - 1;
    float *const shared = reinterpret_cast<float *>(dm_lds);  // [16]: the pose and level this iteration runs with, then the feature table
    uint32_t *const shared_u = reinterpret_cast<uint32_t *>(dm_lds);
    float4 *const feat = dm_lds + 4;
    const float inv_patch_cols = 1.0f / (float)pp.patch_cols;
    const int stride_chunks = np * kDmWaves;
    const int step_i = (int)(((long long)stride_chunks * kDmChunk) / P), step_pix = (int)(((long long)stride_chunks * kDmChunk) % P);
    int cur_level = -1;
    float fx = 0.0f, fy = 0.0f, cx = 0.0f, cy = 0.0f;
    DevImage ref = pr.ref[0], cur = pr.cur[0];
    uint32_t last_tag = 0;
    for (;;) {
        // ---- the next published pose (one wave polls; the others get it through LDS behind the barrier).  Tags only grow; a producer
        // whose waves own no chunk of a small stream may miss one — the consumer does not wait for it — and simply takes the next.
        if (wave == 0) {
            uint32_t seen = last_tag;
            bool ok = false;
            for (uint32_t polls = 0; polls < kSpreadMaxPolls; ++polls) {
                seen = spread_load(header);
                if (seen != last_tag) {
                    ok = true;
                    spread_acquired();
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            const uint32_t mine = lane < 11 ? spread_load(header + lane) : 0u;  // the wave that polled loads what the tag guards
            if (lane >= 2 && lane < 11) {
                shared_u[lane] = mine;
            }
            if (lane == 0) {
                shared_u[0] = ok ? seen : kSpreadStop;
            }
        }
        __syncthreads();
        const uint32_t tag = shared_u[0];
        if (tag == kSpreadStop) {
            break;
        }
        last_tag = tag;
        const int level = (int)shared_u[2];
        Quat q = {shared[4], shared[5], shared[6], shared[7]};
        const float px = shared[8], py = shared[9], pz = shared[10];
        if (level != cur_level) {
            cur_level = level;
            ref = pp.problems[problem].ref[level];
            cur = pp.problems[problem].cur[level];
            const float up = (float)(1 << (pp.n_levels - 1 - level));
            fx = (pr.K[0] / scale) * up;
            fy = (pr.K[1] / scale) * up;
            cx = (pr.K[2] / scale) * up;
            cy = (pr.K[3] / scale) * up;
            for (int i = tid; i < n_track; i += kDmWaves * kWave) {
                dm_level_row(feat, pr, i, scale, up, fx, fy);
            }
        }
        const Quat q_inv = q_inverse(q);
        for (int i = tid; i < n_track; i += kDmWaves * kWave) {
            dm_project(feat, pr, i, q_inv, px, py, pz, fx, fy, cx, cy, producer == 0);
        }
        __syncthreads();
        // ---- this wave's chunks of the stream ----
        int chunk = producer * kDmWaves + wave;
        int ti, tpix;
        {
            const long long t = (long long)chunk * kDmChunk + lane;
            ti = (int)(t / P);
            tpix = (int)(t - (long long)ti * P);
        }
        for (; chunk < n_chunks; chunk += stride_chunks) {
            float jac[6], residual;
            dm_term(feat, pp, ref, cur, ti < n_track, ti, tpix, inv_patch_cols, jac, residual);
            uint32_t *dst = values + (size_t)chunk * (kSpreadValues * kDmChunk) + lane;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                spread_store(dst + r * kDmChunk, __float_as_uint(jac[r]));
            }
            spread_store(dst + 6 * kDmChunk, __float_as_uint(residual));
            spread_stores_done();
            if (lane == 0) {
                spread_publish(chunk_flag + chunk, tag);
            }
            ti += step_i;
            tpix += step_pix;
            if (tpix >= P) {
                tpix -= P;
                ++ti;
            }
        }
        __syncthreads();  // every wave is done with the feature table before the next iteration's projection rewrites it
    }
    // ---- status write-back (:72-83), by the producer that wrote cur_pixel_uv ----
    if (producer == 0) {
        const DevImage bottom = pr.ref[0];
        for (int i = tid; i < n; i += kDmWaves * kWave) {
            uint8_t st = pr.status_valid ? pr.status[i] : (uint8_t)FTK_TRACKED;
            const float u = pr.cur_uv[2 * i], v = pr.cur_uv[2 * i + 1];
            if (u < 0.0f || u > (float)(bottom.cols - 1) || v < 0.0f || v > (float)(bottom.rows - 1)) {
                st = FTK_OUTSIDE;
            }
            pr.status[i] = st;
        }
    }
}

}  // namespace

size_t direct_lds_bytes(uint32_t max_features) {
    return sizeof(float) * ((size_t)2 * kDmProducers * kDmTerms * kDmRow + 96 + 16 * (size_t)max_features);
}

size_t direct_spread_ws_bytes(uint32_t n_track, int32_t patch_rows, int32_t patch_cols) {
    const long long total_terms = (long long)n_track * patch_rows * patch_cols;
    const long long n_chunks = (total_terms + kDmChunk - 1) / kDmChunk;
    return sizeof(uint32_t) * (size_t)(kSpreadHeaderWords + ((n_chunks + 63) & ~63ll) + n_chunks * (long long)(kSpreadValues * kDmChunk));
}

size_t direct_spread_clear_bytes(uint32_t n_track, int32_t patch_rows, int32_t patch_cols) {
    const long long total_terms = (long long)n_track * patch_rows * patch_cols;
    const long long n_chunks = (total_terms + kDmChunk - 1) / kDmChunk;
    return sizeof(uint32_t) * (size_t)(kSpreadHeaderWords + ((n_chunks + 63) & ~63ll));  // header + chunk flags: zero before every launch
}

// How many workgroups of the spread kernel the device can hold AT ONCE (the consumer and its producers wait for each other, so a
// launch that is not co-resident cannot finish: its bounded waits run out and the pose is poisoned).  Occupancy per compute unit
// from the runtime (LDS and registers as launched) x the compute units this process sees — 256 on a whole MI355X, 32 on a CPX partition.
int direct_spread_resident_groups(uint32_t max_features, int device) {
    const size_t lds = direct_lds_bytes(max_features);
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(direct_track_spread_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        return 0;
    }
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, direct_track_spread_kernel, kDmWaves * kWave, lds) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        return 0;
    }
    return per_cu * cus;
}

hipError_t direct_track_launch(const DirectPlan &plan, const DirectParams &p, hipStream_t stream) {
    void (*kernel)(const DirectParams) = p.tree ? direct_track_kernel<true> : direct_track_kernel<false>;
    if (plan.producers > 0) {
        if (p.tree || !p.spread_ws || p.spread_ws_words == 0) {
            return hipErrorInvalidValue;
        }
        kernel = direct_track_spread_kernel;
    }
    if (plan.lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds);
        if (e != hipSuccess) {
            return e;
        }
    }
    hipLaunchKernelGGL(kernel, plan.grid, plan.block, plan.lds, stream, p);
    return hipGetLastError();
}

// First-use cost out of the callers' timed regions (ftk_warmup): launching this empty kernel makes the runtime load this
// translation unit's code object onto the device, which otherwise happens inside the first real call.
__global__ void direct_warm_kernel() {}
hipError_t direct_warm(hipStream_t stream) {
    hipLaunchKernelGGL(direct_warm_kernel, dim3(1), dim3(64), 0, stream);
    return hipGetLastError();
}

}  // namespace ftk
