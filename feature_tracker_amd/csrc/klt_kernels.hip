// klt_kernels.hip — pyramidal Lucas-Kanade trackers for gfx950 (MI355X), hand-written HIP.
//
// One workgroup of W wavefronts (W = 1..4, chosen from the patch size) owns one feature for the
// whole call: it walks the pyramid coarse -> fine and runs every Gauss-Newton iteration without
// leaving the CU, so a TrackFeatures call is ONE launch.  The pyramids of both frames total
// 0.8-5.5 MB and stay L2 / Infinity-Cache resident; per level each workgroup copies the
// (2h+4)^2-pixel footprint of its feature from the reference image, and a slightly larger one from
// the current image, into LDS ("windows", stored as 16-bit pixel pairs so one bilinear sample is
// two ds_read_u16 + four v_cvt_f32_ubyte), and every sample of the Gauss-Newton loop is served from
// there.  Samples that fall outside a window (diverging features, strongly warped patches) take a
// global-memory path with identical arithmetic.
//
// Work split per iteration:
//   phase A (64*W lanes): each lane handles patch pixels tid, tid+64W, ...: bilinear samples,
//                         gradients, residual, and the per-pixel PRODUCTS of every normal-equation
//                         entry, written to LDS as terms[k][pixel].
//   phase B (K lanes)   : lane k < K of wave 0 adds terms[k][0..P) strictly in row-major pixel order
//                         (ds_read_b128 + 4 dependent v_add_f32).  This is the reference's
//                         sequential accumulation order, so sums are bit-identical to the scalar
//                         CPU path; the Gauss-Newton convergence test (||v||^2 < 4e-2) amplifies
//                         any 1-ulp deviation into extra/missing iterations, which is why a
//                         shuffle-tree reduction is not used here.
//   phase C (uniform)   : the K sums are broadcast through LDS, every lane solves the 2x2 / 3x3 /
//                         6x6 system with an Eigen-compatible pivoted LDLT held in registers and
//                         applies the update and the status logic redundantly (no divergence).
//
// Arithmetic contract: IEEE fp32, no FMA contraction (-ffp-contract=off), correctly rounded
// division / sqrt, bilinear weights and summation order exactly as the reference writes them.
//
// Reference behaviour implemented here (file:line relative to the reference repo):
//   basic_klt.cpp:7-181, basic_klt_fast.cpp:7-195, affine_klt.cpp:6-273, affine_klt_fast.cpp:7-188,
//   lssd_klt.cpp:7-250, lssd_klt_fast.cpp:7-229, optical_flow.cpp:49-102.
#include "ftk_device.h"

// Chain prefetch depth: two ping-pong sets of 4 x ds_read_b128 (16 terms, ~144 cycles of dependent adds) cover the
// LDS latency; the default of 8 costs 32 more VGPRs in every variant (basic 104 -> 72, lssd fast 111 -> 85, affine
// inverse 134 -> 122, which then fits 4 waves per SIMD instead of 3).
#define FTK_CHAIN_ROUND 4
#include "klt_chain.h"
#include "klt_ldlt.h"
#include "klt_order.h"
#include "klt_plan.h"
#include "klt_scalar.h"
#include "klt_stage.h"
#include "klt_window.h"

#include <type_traits>

namespace ftk {
namespace {

// ---------------------------------------------------------------------------------------------
// LDS carve-up of one workgroup (dynamic shared memory)
// ---------------------------------------------------------------------------------------------
struct Carve {
    float *terms;         // [K][Ppad] per-pixel products, k-major
    float *a0;            // a0_floats = max(Epad, 12 * (patch_rows + patch_cols)) floats: extended patch / axis tables / i_cur
    float *a1;            // Ppad floats each
    float *a2;
    float *a3;
    float *sums;          // 72 floats: [0,K) chain sums, [K..] published solution, [32,68) affine-fast Hessian
    uint32_t *wave_cnt;   // 24 slots: per-wave valid counts (2 x 4 by parity), miss flags (2 x 4 by parity, + 2 x 4 for the level setup)
    uint16_t *ref_win;    // reference-image window (rwin_rows x rwin_cols pixel pairs)
    uint16_t *cur_win;    // current-image window   (cwin_rows x cwin_cols pixel pairs)
    uint8_t *flagsE;      // Epad bytes
    uint8_t *flagsP;      // Ppad bytes
};

__host__ __device__ inline int pad4(int x) { return (x + 3) & ~3; }

// Per-pixel floats after a0 (KltParams::px_floats): 3 = dx, dy, one more array; 4 = one float4 record per pixel (non-fast affine);
// 6 = a float4 record + a float2 coordinate pair (chunked LSSD).
__host__ __device__ inline int carve_px_floats(const KltParams &p) { return p.px_floats; }

__host__ __device__ inline size_t carve_bytes(int K, const KltParams &p) {
    const size_t epad = (size_t)pad4(p.E);
    const size_t floats = (size_t)(p.terms_floats > 0 ? p.terms_floats : K * p.Ppad) + (size_t)p.a0_floats + (size_t)carve_px_floats(p) * (size_t)p.Ppad + 72 + 24;
    const size_t shorts = (size_t)pad4(p.rwin_rows * p.rwin_cols) + (size_t)pad4(p.cwin_rows * p.cwin_cols);
    return sizeof(float) * floats + sizeof(uint16_t) * shorts + epad + (size_t)p.Ppad;
}

__device__ __forceinline__ Carve carve_lds(float *base, int K, const KltParams &p) {
    Carve c;
    const int epad = pad4(p.E);
    c.terms = base;
    c.a0 = c.terms + (p.terms_floats > 0 ? p.terms_floats : K * p.Ppad);
    c.a1 = c.a0 + p.a0_floats;
    c.a2 = c.a1 + p.Ppad;
    c.a3 = c.a2 + p.Ppad;
    c.sums = c.a1 + carve_px_floats(p) * p.Ppad;
    c.wave_cnt = reinterpret_cast<uint32_t *>(c.sums + 72);
    c.ref_win = reinterpret_cast<uint16_t *>(c.wave_cnt + 24);
    c.cur_win = c.ref_win + pad4(p.rwin_rows * p.rwin_cols);
    c.flagsE = reinterpret_cast<uint8_t *>(c.cur_win + pad4(p.cwin_rows * p.cwin_cols));
    c.flagsP = c.flagsE + epad;
    return c;
}

// The large-patch form (KltParams::spill): the arrays whose size grows with the patch live in this workgroup's slice of device
// memory (`spill`), the fixed-size ones and the image windows in LDS.  Same fields, same order of use; the kernels never ask which.
constexpr int kSpillSlackFloats = 64;  // what the chain's prefetch may read past the last product row

__host__ __device__ inline size_t spill_floats(int K, const KltParams &p) {
    const size_t epad = (size_t)pad4(p.E);
    const size_t floats = (size_t)(p.terms_floats > 0 ? p.terms_floats : K * p.Ppad) + (size_t)p.a0_floats + (size_t)carve_px_floats(p) * (size_t)p.Ppad;
    return floats + (epad + (size_t)p.Ppad + 3) / 4 + kSpillSlackFloats;
}

__host__ __device__ inline size_t spill_lds_bytes(const KltParams &p) {
    // a disabled window (rows 1, cols 0: klt_plan.cpp's choice when the windows do not fit either) still owns eight shorts: the
    // branch-free taps read element 0 before they discard the value
    const size_t shorts = (size_t)pad4(p.rwin_rows * p.rwin_cols) + (size_t)pad4(p.cwin_rows * p.cwin_cols) + 16;
    return sizeof(float) * (72 + 24) + sizeof(uint16_t) * shorts;
}

__device__ __forceinline__ Carve carve_spill(float *lds, float *spill, int K, const KltParams &p) {
    Carve c;
    const int epad = pad4(p.E);
    c.terms = spill;
    c.a0 = c.terms + (p.terms_floats > 0 ? p.terms_floats : K * p.Ppad);
    c.a1 = c.a0 + p.a0_floats;
    c.a2 = c.a1 + p.Ppad;
    c.a3 = c.a2 + p.Ppad;
    c.flagsE = reinterpret_cast<uint8_t *>(c.a1 + carve_px_floats(p) * p.Ppad);
    c.flagsP = c.flagsE + epad;
    c.sums = lds;
    c.wave_cnt = reinterpret_cast<uint32_t *>(c.sums + 72);
    c.ref_win = reinterpret_cast<uint16_t *>(c.wave_cnt + 24);
    c.cur_win = c.ref_win + pad4(p.rwin_rows * p.rwin_cols) + 8;
    return c;
}

// Workgroup-wide sum of the per-wave valid-pixel counts.  The leading barrier also publishes the
// terms written in phase A; the trailing one lets the slots be reused.
__device__ __forceinline__ uint32_t block_total(const Blk &b, uint32_t wave_sum, uint32_t *slots) {
    if (b.solo) {
        blk_sync(b);  // keeps the "terms are published" ordering the callers rely on
        return wave_sum;
    }
    if (b.lane == 0) {
        slots[b.wave] = wave_sum;
    }
    blk_sync(b);
    uint32_t total = 0;
    for (int w = 0; w < b.nwaves; ++w) {
        total += slots[w];
    }
    blk_sync(b);
    return total;
}

// Cheaper form for the per-iteration count: the per-wave counts ride on the two barriers of
// chain_sums (publish before, collect after).  Slots are double-buffered by iteration parity because
// a fast wave may publish its next count before a slow wave has collected the previous one.
__device__ __forceinline__ void publish_count(const Blk &b, uint32_t wave_sum, uint32_t *slots, uint32_t parity) {
    if (b.lane == 0) {
        slots[(parity & 1u) * 4 + b.wave] = wave_sum;
    }
}
// Workgroup-wide OR of a per-lane flag with ONE barrier (which also publishes whatever phase A
// stored before it): wave ballots go to parity-indexed slots, every lane reads them back.
// `bank` selects one of four 4-slot groups so that back-to-back uses never share slots without a
// barrier in between (0 / 1: iteration parity, 2 / 3: level setup fast / slow pass).
__device__ __forceinline__ bool block_any(const Blk &b, bool flag, uint32_t *slots, uint32_t bank) {
    const bool wave_any = wave_ballot(flag) != 0ull;
    if (b.solo) {
        blk_sync(b);
        return wave_any;
    }
    if (b.lane == 0) {
        slots[8 + bank * 4 + b.wave] = wave_any ? 1u : 0u;
    }
    blk_sync(b);
    uint32_t any = 0;
    for (int w = 0; w < b.nwaves; ++w) {
        any |= slots[8 + bank * 4 + w];
    }
    return any != 0;
}

__device__ __forceinline__ uint32_t collect_count(const Blk &b, const uint32_t *slots, uint32_t parity) {
    uint32_t total = 0;
    for (int w = 0; w < b.nwaves; ++w) {
        total += slots[(parity & 1u) * 4 + w];
    }
    return total;
}

// The chunked LSSD levels leave sum k in lane 4 k when they ran the quad chains (KltParams::quad_chain), in lane k otherwise.
__device__ __forceinline__ int sum_lanes(const KltParams &p) { return p.quad_chain ? 4 : 1; }

// The K <= 16 sums of `terms[K][Ppad]` by ALL lanes of one wave: quad q = lanes 4 q .. 4 q + 3 carries sum q (the quads behind the last
// sum follow its row and are ignored), Ppad / 16 steps of 16 ordered adds each; lane 4 q publishes sum q.  Same adds, same order as
// chain_lane on lane q.  Ppad is a multiple of 16 and the rows' padding holds exact zeros (klt_fill_geometry, zero_term_padding).
__device__ __forceinline__ void chain_rows_quads(const float *terms, int K, int Ppad, float *sums, int lane) {
    const int q = lane >> 2;
    const float acc = chain_quads_row(0.0f, terms + (q < K ? q : K - 1) * Ppad + 4 * (lane & 3), Ppad >> 4);
    if ((lane & 3) == 0 && q < K) {
        sums[q] = acc;
    }
}

__device__ __forceinline__ void chain_sums(const Blk &b, const float *terms, int K, int Ppad, float *sums, bool leading_barrier = false) {
    if (leading_barrier) {
        blk_sync(b);  // phase A's terms (and published counts) become visible
    }
    if (b.wave == 0) {
        if (b.tree) {
            tree_sums(terms, K, Ppad, sums, b.lane);  // throughput mode: not the reference's order
        } else if (K <= 16) {
            chain_rows_quads(terms, K, Ppad, sums, b.lane);
        } else if (b.lane < K) {
            sums[b.lane] = chain_lane(terms + b.lane * Ppad, Ppad);
        }
    }
    blk_sync(b);
}

// Phase B + C on wave 0 only: after its chain lanes have published the K sums, wave 0 runs
// `wave0_work` (the small dense solve) and publishes the solution through LDS; one barrier releases
// the other waves, which were idle during the chain anyway.  Within one wave LDS operations execute
// in program order, so wave 0 needs no barrier between its own chain stores and solve loads.
template <typename F>
__device__ __forceinline__ void chain_then(const Blk &b, const float *terms, int K, int Ppad, float *sums, bool leading_barrier, F &&wave0_work) {
    if (leading_barrier) {
        blk_sync(b);  // phase A's terms (and published counts) become visible
    }
    if (b.wave == 0) {
        if (b.tree) {
            tree_sums(terms, K, Ppad, sums, b.lane);  // throughput mode: not the reference's order
            __builtin_amdgcn_wave_barrier();
        } else if (K <= 16) {
            chain_rows_quads(terms, K, Ppad, sums, b.lane);
        } else if (b.lane < K) {
            sums[b.lane] = chain_lane(terms + b.lane * Ppad, Ppad);
        }
        wave0_work();
    }
    blk_sync(b);
}

__device__ __forceinline__ void zero_term_padding(const Blk &b, float *terms, int K, const KltParams &p) {
    const int extra = p.Ppad - p.P;
    for (int idx = b.tid; idx < K * extra; idx += b.nt) {
        const int k = idx / (extra > 0 ? extra : 1);
        terms[k * p.Ppad + p.P + (idx - k * extra)] = 0.0f;
    }
}

// Both level windows inside their images: every thread issues the 8-byte loads of its reference
// quads AND its current quads before the first LDS store, so the two global round trips overlap.
__device__ __forceinline__ void stage_both_inside(const Blk &b, const KltParams &p, const DevImage &ref, const DevImage &cur, const Win &rw,
                                                  const Win &cw, Carve &c) {
    const int rq = rw.cols >> 2, cq = cw.cols >> 2;
    const int total_r = rw.rows * rq, total_c = cw.rows * cq;  // total_c >= total_r
    for (int base = 0; base < total_c; base += 2 * b.nt) {
        const int i0 = base + b.tid, i1 = base + b.nt + b.tid;
        int or0, or1, oc0, oc1;
        const uint2 vr0 = load_quad_pairs(ref, rw.r_lo, rw.c_lo, i0 < total_r ? i0 : 0, rq, p.magic_rwq, or0, rw.cols);
        const uint2 vr1 = load_quad_pairs(ref, rw.r_lo, rw.c_lo, i1 < total_r ? i1 : 0, rq, p.magic_rwq, or1, rw.cols);
        const uint2 vc0 = load_quad_pairs(cur, cw.r_lo, cw.c_lo, i0 < total_c ? i0 : 0, cq, p.magic_cwq, oc0, cw.cols);
        const uint2 vc1 = load_quad_pairs(cur, cw.r_lo, cw.c_lo, i1 < total_c ? i1 : 0, cq, p.magic_cwq, oc1, cw.cols);
        if (i0 < total_r) {
            *reinterpret_cast<uint2 *>(c.ref_win + or0) = vr0;
        }
        if (i1 < total_r) {
            *reinterpret_cast<uint2 *>(c.ref_win + or1) = vr1;
        }
        if (i0 < total_c) {
            *reinterpret_cast<uint2 *>(c.cur_win + oc0) = vc0;
        }
        if (i1 < total_c) {
            *reinterpret_cast<uint2 *>(c.cur_win + oc1) = vc1;
        }
    }
}

// Level entry: stages the reference footprint of (ref_u, ref_v) and the current footprint (+ margin)
// of (cur_u, cur_v) back to back with a single barrier, so the global round trips overlap.
__device__ __forceinline__ void stage_level_windows(const Blk &b, const KltParams &p, const DevImage &ref, const DevImage &cur, float ref_u,
                                                    float ref_v, float cur_u, float cur_v, Carve &c, Win &rw, Win &cw, int ref_axis_variants = 0) {
    footprint_origin(p, ref_u, ref_v, rw.r_lo, rw.c_lo);
    rw.rows = p.rwin_rows;
    rw.cols = p.rwin_cols;
    rw.data = c.ref_win;
    int need_r, need_c;
    footprint_origin(p, cur_u, cur_v, need_r, need_c);
    cw.r_lo = wadd(need_r, -p.cwin_margin);
    cw.c_lo = wadd(need_c, -p.cwin_margin);
    cw.rows = p.cwin_rows;
    cw.cols = p.cwin_cols;
    cw.data = c.cur_win;
    win_set_cover(p, cw);
    if (ref_axis_variants > 0) {
        build_axis_tables(b, p, ref, rw, ref_u, ref_v, ref_axis_variants, reinterpret_cast<float4 *>(c.a0));
    }
    if (window_inside(ref, rw.r_lo, rw.c_lo, rw.rows, rw.cols) && window_inside(cur, cw.r_lo, cw.c_lo, cw.rows, cw.cols)) {
        stage_both_inside(b, p, ref, cur, rw, cw, c);
    } else {
        stage_any(b, ref, c.ref_win, rw.r_lo, rw.c_lo, rw.rows, rw.cols, p.magic_rwc, p.magic_rwq);
        stage_any(b, cur, c.cur_win, cw.r_lo, cw.c_lo, cw.rows, cw.cols, p.magic_cwc, p.magic_cwq);
    }
    blk_sync(b);
}

// Makes sure the current-image window covers the footprint of a patch centred at (u, v); restages
// it (with cwin_margin pixels of slack on every side) when it does not.  Wave-uniform decision.
__device__ __forceinline__ void ensure_cur_window(const Blk &b, const KltParams &p, const DevImage &cur, float u, float v, Carve &c, Win &w,
                                                  bool &staged) {
    if (staged && win_covers(w, u, v)) {
        return;  // the usual case: a handful of compares (NaN and huge coordinates fail them and take the integer test below)
    }
    int need_r, need_c;
    footprint_origin(p, u, v, need_r, need_c);
    const long long nr = need_r, nc = need_c;
    const bool covered = staged && nr >= (long long)w.r_lo && nr + (2 * p.half_rows + 4) <= (long long)w.r_lo + w.rows &&
                         nc >= (long long)w.c_lo && nc + (2 * p.half_cols + 4) <= (long long)w.c_lo + w.cols + 1;
    if (!covered) {
        w.r_lo = wadd(need_r, -p.cwin_margin);
        w.c_lo = wadd(need_c, -p.cwin_margin);
        w.rows = p.cwin_rows;
        w.cols = p.cwin_cols;
        w.data = c.cur_win;
        win_set_cover(p, w);
        stage_any(b, cur, c.cur_win, w.r_lo, w.c_lo, w.rows, w.cols, p.magic_cwc, p.magic_cwq);
        blk_sync(b);
        staged = true;
    }
}

// ---------------------------------------------------------------------------------------------
// Shared pieces of the non-fast variants (inverse / direct)
//   a1 = gx (right - left), a2 = gy (bottom - top), a3 = i_ref, flagsP = ref-side validity.
// For METHOD == inverse the five reference-image fetches of a pixel do not change within a
// level, so they are sampled once per level; the arithmetic per pixel is unchanged.
// ---------------------------------------------------------------------------------------------
// SLOW = false: straight-line taps from the axis tables; a pixel whose taps are not all covered by
// the staged window only raises `miss` (returned workgroup-wide).  SLOW = true: every sample goes
// through the general sampler (LDS window or global memory, identical arithmetic).  The slow pass
// is a separate loop, so the hot loop carries no fallback code.
// PACKED: what an iteration reads of a pixel — {gx, gy, i_ref, used} — goes into ONE float4 at a1 (px_floats == 4) instead of three
// float arrays and a byte array: one 16-byte read and one address per pixel and iteration instead of four.
template <int METHOD, bool SLOW, bool PACKED>
__device__ __forceinline__ bool nonfast_setup_pass(const Blk &b, const KltParams &p, const DevImage &ref, const Win &rw, float ref_u, float ref_v,
                                                   Carve &c) {
    const float4 *tab = reinterpret_cast<const float4 *>(c.a0);
    const int variants = (METHOD == FTK_METHOD_INVERSE) ? 3 : 1;
    const float4 *rows0 = tab, *rowsm = tab + p.patch_rows, *rowsp = tab + 2 * p.patch_rows;
    const float4 *cols0 = tab + variants * p.patch_rows, *colsm = cols0 + p.patch_cols, *colsp = cols0 + 2 * p.patch_cols;
    bool miss = false;
    for (int pxi = b.tid; pxi < p.P; pxi += b.nt) {
        int prow, pcol;
        pixel_rc(p, pxi, prow, pcol);
        float left = 0.0f, right = 0.0f, top = 0.0f, bottom = 0.0f, i_ref = 0.0f;
        bool ok;
        if (SLOW) {
            const float row_i = (float)(prow - p.half_rows) + ref_v;
            const float col_i = (float)(pcol - p.half_cols) + ref_u;
            if (METHOD == FTK_METHOD_INVERSE) {
                ok = sample(ref, rw, row_i, col_i - 1.0f, left) && sample(ref, rw, row_i, col_i + 1.0f, right) &&
                     sample(ref, rw, row_i - 1.0f, col_i, top) && sample(ref, rw, row_i + 1.0f, col_i, bottom) && sample(ref, rw, row_i, col_i, i_ref);
            } else {
                ok = sample(ref, rw, row_i, col_i, i_ref);
            }
        } else {
            const float4 r0 = rows0[prow], c0 = cols0[pcol];
            int flags;
            if (METHOD == FTK_METHOD_INVERSE) {
                const float4 rm = rowsm[prow], rp = rowsp[prow], cm = colsm[pcol], cp = colsp[pcol];
                flags = __float_as_int(r0.w) & __float_as_int(c0.w) & __float_as_int(rm.w) & __float_as_int(rp.w) & __float_as_int(cm.w) &
                        __float_as_int(cp.w);
                left = tap_table(rw, r0, cm);
                right = tap_table(rw, r0, cp);
                top = tap_table(rw, rm, c0);
                bottom = tap_table(rw, rp, c0);
                i_ref = tap_table(rw, r0, c0);
            } else {
                flags = __float_as_int(r0.w) & __float_as_int(c0.w);
                i_ref = tap_table(rw, r0, c0);
            }
            ok = (flags & 1) != 0;
            miss = miss || (flags == 1);  // inside the image but not inside the staged window
        }
        if (PACKED) {
            reinterpret_cast<float4 *>(c.a1)[pxi] = make_float4(right - left, bottom - top, i_ref, __int_as_float(ok ? -1 : 0));
        } else {
            if (METHOD == FTK_METHOD_INVERSE) {
                c.a1[pxi] = right - left;
                c.a2[pxi] = bottom - top;
            }
            c.a3[pxi] = i_ref;
            c.flagsP[pxi] = ok ? 1 : 0;
        }
    }
    return block_any(b, miss, c.wave_cnt, SLOW ? 3u : 2u);
}

template <int METHOD, bool PACKED = false>
__device__ __forceinline__ void nonfast_level_setup(const Blk &b, const KltParams &p, const DevImage &ref, const Win &rw, float ref_u, float ref_v,
                                                    Carve &c) {
    if (nonfast_setup_pass<METHOD, false, PACKED>(b, p, ref, rw, ref_u, ref_v, c)) {
        nonfast_setup_pass<METHOD, true, PACKED>(b, p, ref, rw, ref_u, ref_v, c);
    }
}

// Completes the six fetches of one patch pixel for the current iteration.
//   MODE 0: straight-line taps, a tap outside the window only raises `miss` (caller redoes the phase)
//   MODE 1: every sample through the general sampler
//   MODE 2: straight-line taps with a per-pixel redo through the general sampler (for warped patches,
//           whose corner taps leave the window now and then: cheaper than redoing the whole phase)
enum { kGatherHoisted = 0, kGatherGeneral = 1, kGatherInline = 2 };

template <int METHOD, int MODE, bool PACKED = false>
__device__ __forceinline__ bool nonfast_gather(const DevImage &cur, const Win &cw, const Carve &c, int pxi, float row_j, float col_j, float &gx,
                                               float &gy, float &i_ref, float &i_cur, bool &miss) {
    bool ok;
    float gx_ref, gy_ref;
    if (PACKED) {
        const float4 rec = reinterpret_cast<const float4 *>(c.a1)[pxi];
        gx_ref = rec.x;
        gy_ref = rec.y;
        i_ref = rec.z;
        ok = __float_as_int(rec.w) != 0;
    } else {
        ok = c.flagsP[pxi] != 0;
        i_ref = c.a3[pxi];
        gx_ref = (METHOD == FTK_METHOD_INVERSE) ? c.a1[pxi] : 0.0f;
        gy_ref = (METHOD == FTK_METHOD_INVERSE) ? c.a2[pxi] : 0.0f;
    }
    i_cur = 0.0f;
    if (MODE == kGatherGeneral) {
        if (METHOD == FTK_METHOD_INVERSE) {
            gx = gx_ref;
            gy = gy_ref;
            ok = sample(cur, cw, row_j, col_j, i_cur) && ok;
        } else {
            float left = 0.0f, right = 0.0f, top = 0.0f, bottom = 0.0f;
            const bool g = sample(cur, cw, row_j, col_j - 1.0f, left) && sample(cur, cw, row_j, col_j + 1.0f, right) &&
                           sample(cur, cw, row_j - 1.0f, col_j, top) && sample(cur, cw, row_j + 1.0f, col_j, bottom) && sample(cur, cw, row_j, col_j, i_cur);
            gx = right - left;
            gy = bottom - top;
            ok = ok && g;
        }
        return ok;
    }
    const Axis r0 = make_axis(row_j, cur.rows - 1), c0 = make_axis(col_j, cur.cols - 1);
    bool hit = true;
    bool valid;
    if (METHOD == FTK_METHOD_INVERSE) {
        gx = gx_ref;
        gy = gy_ref;
        valid = r0.valid && c0.valid;
        i_cur = tap(cw, r0, c0, hit);
        if (MODE == kGatherInline && valid && !hit) {
            sample(cur, cw, row_j, col_j, i_cur);
        }
    } else {
        const Axis rm = make_axis(row_j - 1.0f, cur.rows - 1), rp = make_axis(row_j + 1.0f, cur.rows - 1);
        const Axis cm = make_axis(col_j - 1.0f, cur.cols - 1), cp = make_axis(col_j + 1.0f, cur.cols - 1);
        valid = r0.valid && c0.valid && rm.valid && rp.valid && cm.valid && cp.valid;
        float left = tap(cw, r0, cm, hit);
        float right = tap(cw, r0, cp, hit);
        float top = tap(cw, rm, c0, hit);
        float bottom = tap(cw, rp, c0, hit);
        i_cur = tap(cw, r0, c0, hit);
        if (MODE == kGatherInline && valid && !hit) {
            sample(cur, cw, row_j, col_j - 1.0f, left);
            sample(cur, cw, row_j, col_j + 1.0f, right);
            sample(cur, cw, row_j - 1.0f, col_j, top);
            sample(cur, cw, row_j + 1.0f, col_j, bottom);
            sample(cur, cw, row_j, col_j, i_cur);
        }
        gx = right - left;
        gy = bottom - top;
    }
    if (MODE == kGatherHoisted) {
        miss = miss || (valid && !hit);
    }
    return ok && valid;
}

// ---------------------------------------------------------------------------------------------
// Shared pieces of the fast variants
//   a0 = extended reference patch (E), flagsE = its validity, a1 = dx (P), a2 = dy (P)
// ---------------------------------------------------------------------------------------------

// OpticalFlow::ExtractExtendPatchInReferenceImage (optical_flow.cpp:49-102); returns the valid count.
__device__ __forceinline__ uint32_t extract_extended_patch(const Blk &b, const KltParams &p, const DevImage &ref, const Win &rw, float ref_u,
                                                           float ref_v, Carve &c) {
    float *ex = c.a0;
    uint8_t *exv = c.flagsE;
    const float int_row = floorf(ref_v);
    const float int_col = floorf(ref_u);
    const float dec_row = ref_v - int_row;
    const float dec_col = ref_u - int_col;
    const float w_tl = (1.0f - dec_row) * (1.0f - dec_col);
    const float w_tr = (1.0f - dec_row) * dec_col;
    const float w_bl = dec_row * (1.0f - dec_col);
    const float w_br = dec_row * dec_col;
    const int min_row = wadd(f2i(int_row), -(p.ex_rows / 2));
    const int min_col = wadd(f2i(int_col), -(p.ex_cols / 2));
    uint32_t count = 0;
    for (int base = 0; base < p.E; base += b.nt) {
        const int e = base + b.tid;
        bool valid = false;
        if (e < p.E) {
            const int erow = (int)__umulhi((unsigned)e, p.magic_exc);
            const int ecol = e - imul(erow, p.ex_cols);
            const int row = wadd(min_row, erow);
            const int col = wadd(min_col, ecol);
            valid = !(row < 0 || row > ref.rows - 2 || col < 0 || col > ref.cols - 2);
            float value = 0.0f;
            if (valid) {
                float p00, p01, p10, p11;
                fetch4(ref, rw, row, col, p00, p01, p10, p11);
                value = w_tl * p00 + w_tr * p01 + w_bl * p10 + w_br * p11;
            }
            ex[e] = value;
            exv[e] = valid ? 1 : 0;
        }
        count += (uint32_t)__popcll(wave_ballot(valid));
    }
    return block_total(b, count, c.wave_cnt);
}

// Central differences on the extended patch: dx = dy = 0 where a 4-neighbour is invalid
// (basic_klt_fast.cpp:64-99, affine_klt_fast.cpp:71-138, lssd_klt_fast.cpp:116-143).
__device__ __forceinline__ bool ex_gradient(const KltParams &p, const float *ex, const uint8_t *exv, int prow, int pcol, float &dx, float &dy) {
    const int ei = imul(prow + 1, p.ex_cols) + pcol + 1;
    if (exv[ei - 1] && exv[ei + 1] && exv[ei - p.ex_cols] && exv[ei + p.ex_cols]) {
        dx = ex[ei + 1] - ex[ei - 1];
        dy = ex[ei + p.ex_cols] - ex[ei - p.ex_cols];
        return true;
    }
    dx = 0.0f;
    dy = 0.0f;
    return false;
}

// ---------------------------------------------------------------------------------------------
// Basic KLT (translation only, 2x2)
// ---------------------------------------------------------------------------------------------
struct BasicState {
    float cur_u, cur_v;
};

// TrackOneFeature, basic_klt.cpp:88-181.  Terms: 0 H00, 1 H11, 2 H01, 3 -fx*ft, 4 -fy*ft.
template <int METHOD>
__device__ __forceinline__ void basic_level(const Blk &b, const KltParams &p, const DevImage &ref, const DevImage &cur, float ref_u, float ref_v,
                                            BasicState &s, uint8_t &status, uint32_t &iters, Carve &c) {
    Win rw, cw;
    stage_level_windows(b, p, ref, cur, ref_u, ref_v, s.cur_u, s.cur_v, c, rw, cw, (METHOD == FTK_METHOD_INVERSE) ? 3 : 1);
    bool cw_staged = true;
    nonfast_level_setup<METHOD>(b, p, ref, rw, ref_u, ref_v, c);
    for (uint32_t iter = 0; iter < p.max_iteration; ++iter) {
        ++iters;
        ensure_cur_window(b, p, cur, s.cur_u, s.cur_v, c, cw, cw_staged);
        // phase A; slow == true_type redoes it through the general sampler when a tap left the window
        auto phase_a = [&](auto slow, bool &miss) -> uint32_t {
            constexpr bool kSlow = decltype(slow)::value;
            uint32_t wave_valid = 0;
            for (int base = 0; base < p.P; base += b.nt) {
                const int pxi = base + b.tid;
                bool ok = false;
                if (pxi < p.P) {
                    int prow, pcol;
                    pixel_rc(p, pxi, prow, pcol);
                    const float row_j = (float)(prow - p.half_rows) + s.cur_v;
                    const float col_j = (float)(pcol - p.half_cols) + s.cur_u;
                    float fx, fy, i_ref, i_cur;
                    ok = nonfast_gather<METHOD, kSlow ? kGatherGeneral : kGatherHoisted>(cur, cw, c, pxi, row_j, col_j, fx, fy, i_ref, i_cur, miss);
                    const float ft = i_cur - i_ref;
                    c.terms[0 * p.Ppad + pxi] = ok ? fx * fx : 0.0f;
                    c.terms[1 * p.Ppad + pxi] = ok ? fy * fy : 0.0f;
                    c.terms[2 * p.Ppad + pxi] = ok ? fx * fy : 0.0f;
                    c.terms[3 * p.Ppad + pxi] = ok ? -(fx * ft) : 0.0f;
                    c.terms[4 * p.Ppad + pxi] = ok ? -(fy * ft) : 0.0f;
                }
                wave_valid += (uint32_t)__popcll(wave_ballot(ok));
            }
            return wave_valid;
        };
        bool miss = false;
        uint32_t n_valid = phase_a(std::false_type{}, miss);
        publish_count(b, n_valid, c.wave_cnt, iter);
        if (block_any(b, miss, c.wave_cnt, iter & 1u)) {
            n_valid = phase_a(std::true_type{}, miss);
            publish_count(b, n_valid, c.wave_cnt, iter);
            blk_sync(b);
        }
        chain_then(b, c.terms, 5, p.Ppad, c.sums, false, [&]() {
            float m[2][2];
            float bb[2], sol[2];
            m[0][0] = c.sums[0];
            m[1][1] = c.sums[1];
            m[0][1] = m[1][0] = c.sums[2];
            bb[0] = c.sums[3];
            bb[1] = c.sums[4];
            ldlt_solve<2>(m, bb, sol);
            c.sums[16] = sol[0];
            c.sums[17] = sol[1];
            reinterpret_cast<uint32_t *>(c.sums)[18] = collect_count(b, c.wave_cnt, iter);  // travels with the solution: one LDS round trip after the barrier
        });
        n_valid = reinterpret_cast<const uint32_t *>(c.sums)[18];
        const float v[2] = {c.sums[16], c.sums[17]};
        if (n_valid == 0) {
            break;
        }
        if (isnan(v[0]) || isnan(v[1])) {
            status = FTK_NUMERIC_ERROR;
            break;
        }
        s.cur_u += v[0];
        s.cur_v += v[1];
        if (uv_outside(s.cur_u, s.cur_v, cur)) {
            status = FTK_OUTSIDE;
            break;
        }
        if (v[0] * v[0] + v[1] * v[1] < p.converge) {
            status = FTK_TRACKED;
            break;
        }
    }
}

// TrackOneFeatureFast, basic_klt_fast.cpp:7-195.
__device__ __forceinline__ void basic_level_fast(const Blk &b, const KltParams &p, const DevImage &ref, const DevImage &cur, float ref_u,
                                                 float ref_v, BasicState &s, uint8_t &status, uint32_t &iters, Carve &c) {
    float *ex = c.a0, *dxs = c.a1, *dys = c.a2;
    uint8_t *exv = c.flagsE;
    Win rw, cw;
    stage_level_windows(b, p, ref, cur, ref_u, ref_v, s.cur_u, s.cur_v, c, rw, cw);
    bool cw_staged = true;
    if (extract_extended_patch(b, p, ref, rw, ref_u, ref_v, c) == 0) {
        status = FTK_OUTSIDE;
        return;
    }
    // dx, dy and the fixed Hessian: terms 0 dx*dx, 1 dx*dy, 2 dy*dy
    for (int pxi = b.tid; pxi < p.P; pxi += b.nt) {
        int prow, pcol;
        pixel_rc(p, pxi, prow, pcol);
        float dx, dy;
        ex_gradient(p, ex, exv, prow, pcol, dx, dy);
        dxs[pxi] = dx;
        dys[pxi] = dy;
        c.terms[0 * p.Ppad + pxi] = dx * dx;
        c.terms[1 * p.Ppad + pxi] = dx * dy;
        c.terms[2 * p.Ppad + pxi] = dy * dy;
    }
    blk_sync(b);
    chain_sums(b, c.terms, 3, p.Ppad, c.sums);
    const float h00 = c.sums[0], h01 = c.sums[1], h11 = c.sums[2];

    status = FTK_LARGE_RESIDUAL;
    float last_squared_step = INFINITY;
    uint32_t large_step_cnt = 0;
    for (uint32_t iter = 0; iter < p.max_iteration; ++iter) {
        ++iters;
        ensure_cur_window(b, p, cur, s.cur_u, s.cur_v, c, cw, cw_staged);
        // ComputeBias (:101-195): one weight set from frac(cur), integer lattice floor(cur) - patch/2
        const float int_row = floorf(s.cur_v);
        const float int_col = floorf(s.cur_u);
        const float dec_row = s.cur_v - int_row;
        const float dec_col = s.cur_u - int_col;
        const float w_tl = (1.0f - dec_row) * (1.0f - dec_col);
        const float w_tr = (1.0f - dec_row) * dec_col;
        const float w_bl = dec_row * (1.0f - dec_col);
        const float w_br = dec_row * dec_col;
        const int min_row = wadd(f2i(int_row), -(p.patch_rows / 2));
        const int min_col = wadd(f2i(int_col), -(p.patch_cols / 2));
        uint32_t n_valid = 0;
        for (int base = 0; base < p.P; base += b.nt) {
            const int pxi = base + b.tid;
            bool ok = false;
            if (pxi < p.P) {
                int prow, pcol;
                pixel_rc(p, pxi, prow, pcol);
                const int row = wadd(min_row, prow);
                const int col = wadd(min_col, pcol);
                const int ei = imul(prow + 1, p.ex_cols) + pcol + 1;
                ok = !(row < 0 || row > cur.rows - 2 || col < 0 || col > cur.cols - 2) && exv[ei] != 0;
                float t0 = 0.0f, t1 = 0.0f;
                if (ok) {
                    float p00, p01, p10, p11;
                    fetch4(cur, cw, row, col, p00, p01, p10, p11);
                    const float i_cur = w_tl * p00 + w_tr * p01 + w_bl * p10 + w_br * p11;
                    const float dt = i_cur - ex[ei];
                    t0 = -(dxs[pxi] * dt);
                    t1 = -(dys[pxi] * dt);
                }
                c.terms[0 * p.Ppad + pxi] = t0;
                c.terms[1 * p.Ppad + pxi] = t1;
            }
            n_valid += (uint32_t)__popcll(wave_ballot(ok));
        }
        publish_count(b, n_valid, c.wave_cnt, iter);
        chain_then(b, c.terms, 2, p.Ppad, c.sums, true, [&]() {
            float m[2][2] = {{h00, h01}, {h01, h11}};
            float bb[2] = {c.sums[0], c.sums[1]};
            float sol[2];
            ldlt_solve<2>(m, bb, sol);
            c.sums[16] = sol[0];
            c.sums[17] = sol[1];
            reinterpret_cast<uint32_t *>(c.sums)[18] = collect_count(b, c.wave_cnt, iter);  // travels with the solution: one LDS round trip after the barrier
        });
        n_valid = reinterpret_cast<const uint32_t *>(c.sums)[18];
        const float v[2] = {c.sums[16], c.sums[17]};
        if (n_valid == 0) {
            break;
        }
        if (isnan(v[0]) || isnan(v[1])) {
            status = FTK_NUMERIC_ERROR;
            break;
        }
        s.cur_u += v[0];
        s.cur_v += v[1];
        if (fast_step_logic(p, v[0] * v[0] + v[1] * v[1], last_squared_step, large_step_cnt, status)) {
            break;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Affine KLT (6x6).  The chain indices A_* of its 18 + 6 sums, affine_dense_slots and kAffineDiagLane live in klt_ldlt.h
// (shared with the one-wave fast kernel, klt_fast_kernels.hip).
// ---------------------------------------------------------------------------------------------
struct AffineState {
    float cur_u, cur_v;
    float a00, a01, a10, a11;
};

__device__ __forceinline__ void affine_hessian_terms(const KltParams &p, float *terms, int pxi, bool ok, float x, float y, float dx, float dy) {
    const float xx = x * x, yy = y * y, xy = x * y;
    const float dxdx = dx * dx, dydy = dy * dy, dxdy = dx * dy;
    terms[A_XX_DXDX * p.Ppad + pxi] = ok ? xx * dxdx : 0.0f;
    terms[A_XX_DXDY * p.Ppad + pxi] = ok ? xx * dxdy : 0.0f;
    terms[A_XY_DXDX * p.Ppad + pxi] = ok ? xy * dxdx : 0.0f;
    terms[A_XY_DXDY * p.Ppad + pxi] = ok ? xy * dxdy : 0.0f;
    terms[A_X_DXDX * p.Ppad + pxi] = ok ? x * dxdx : 0.0f;
    terms[A_X_DXDY * p.Ppad + pxi] = ok ? x * dxdy : 0.0f;
    terms[A_XX_DYDY * p.Ppad + pxi] = ok ? xx * dydy : 0.0f;
    terms[A_XY_DYDY * p.Ppad + pxi] = ok ? xy * dydy : 0.0f;
    terms[A_X_DYDY * p.Ppad + pxi] = ok ? x * dydy : 0.0f;
    terms[A_YY_DXDX * p.Ppad + pxi] = ok ? yy * dxdx : 0.0f;
    terms[A_YY_DXDY * p.Ppad + pxi] = ok ? yy * dxdy : 0.0f;
    terms[A_Y_DXDX * p.Ppad + pxi] = ok ? y * dxdx : 0.0f;
    terms[A_Y_DXDY * p.Ppad + pxi] = ok ? y * dxdy : 0.0f;
    terms[A_YY_DYDY * p.Ppad + pxi] = ok ? yy * dydy : 0.0f;
    terms[A_Y_DYDY * p.Ppad + pxi] = ok ? y * dydy : 0.0f;
    terms[A_DXDX * p.Ppad + pxi] = ok ? dxdx : 0.0f;
    terms[A_DXDY * p.Ppad + pxi] = ok ? dxdy : 0.0f;
    terms[A_DYDY * p.Ppad + pxi] = ok ? dydy : 0.0f;
}

// bias(0) -= dt * x * dx ... (affine_klt.cpp:251-256, affine_klt_fast.cpp:174-179); first_bias_chain
// is A_B0 in the non-fast layout and 0 in the fast one.
__device__ __forceinline__ void affine_bias_terms(const KltParams &p, float *terms, int first_bias_chain, int pxi, bool ok, float dt, float x,
                                                  float y, float dx, float dy) {
    terms[(first_bias_chain + 0) * p.Ppad + pxi] = ok ? -(dt * x * dx) : 0.0f;
    terms[(first_bias_chain + 1) * p.Ppad + pxi] = ok ? -(dt * x * dy) : 0.0f;
    terms[(first_bias_chain + 2) * p.Ppad + pxi] = ok ? -(dt * y * dx) : 0.0f;
    terms[(first_bias_chain + 3) * p.Ppad + pxi] = ok ? -(dt * y * dy) : 0.0f;
    terms[(first_bias_chain + 4) * p.Ppad + pxi] = ok ? -(dt * dx) : 0.0f;
    terms[(first_bias_chain + 5) * p.Ppad + pxi] = ok ? -(dt * dy) : 0.0f;
}

// The 24 products of one pixel of the non-fast affine variants (affine_klt.cpp:229-256).  An unused pixel contributes exact zeros
// to every sum: zeroing the five factors does that with five selects instead of one per product — every product is then +0 or
// -0, and x + (+-0) == x for every value a sum can hold (the sums start at +0, and +0 + (-0) == +0).
//
// Layout: [pixel group of 4][24 sums][4 pixels], groups kAffineGroup floats apart (one float4 of padding spreads the groups over the
// banks).  A pixel lane then writes its 24 products at IMMEDIATE offsets from one address (with the sum-major [24][Ppad] layout
// and its run-time pitch the compiler kept 24 row pointers in registers and spent a VALU instruction on each store), and chain
// lane k still reads four consecutive terms of its sum per ds_read_b128 (chain_groups).
constexpr int kAffineGroup = kAffineTermsGroupFloats;
static_assert(kAffineGroup == 4 * A_COUNT + 4, "ftk_device.h sizes the affine product groups for 24 sums");
// Groups are allocated (and chained) in rounds of kChainRound; the pixels P .. 4 * kChainRound * rounds - 1 hold zeros.
static_assert(kChainRound == kAffineTermsRoundGroups, "ftk_device.h rounds the affine product groups to the chain's prefetch round");
static_assert(kWave % (4 * kChainRound) == 0, "a workgroup's first pass (64 pixels per wave) covers whole rounds");
__device__ __forceinline__ int affine_group_rounds(int Ppad) { return ((Ppad >> 2) + kChainRound - 1) / kChainRound; }

__device__ __forceinline__ void affine_all_terms(float *group_terms, int pxi, bool ok, float dt, float x, float y, float dx, float dy) {
    float *terms = group_terms + imul(pxi >> 2, kAffineGroup) + (pxi & 3);
    x = ok ? x : 0.0f;
    y = ok ? y : 0.0f;
    dx = ok ? dx : 0.0f;
    dy = ok ? dy : 0.0f;
    dt = ok ? dt : 0.0f;
    const float xx = x * x, yy = y * y, xy = x * y;
    const float dxdx = dx * dx, dydy = dy * dy, dxdy = dx * dy;
    terms[4 * (A_XX_DXDX)] = xx * dxdx;
    terms[4 * (A_XX_DXDY)] = xx * dxdy;
    terms[4 * (A_XY_DXDX)] = xy * dxdx;
    terms[4 * (A_XY_DXDY)] = xy * dxdy;
    terms[4 * (A_X_DXDX)] = x * dxdx;
    terms[4 * (A_X_DXDY)] = x * dxdy;
    terms[4 * (A_XX_DYDY)] = xx * dydy;
    terms[4 * (A_XY_DYDY)] = xy * dydy;
    terms[4 * (A_X_DYDY)] = x * dydy;
    terms[4 * (A_YY_DXDX)] = yy * dxdx;
    terms[4 * (A_YY_DXDY)] = yy * dxdy;
    terms[4 * (A_Y_DXDX)] = y * dxdx;
    terms[4 * (A_Y_DXDY)] = y * dxdy;
    terms[4 * (A_YY_DYDY)] = yy * dydy;
    terms[4 * (A_Y_DYDY)] = y * dydy;
    terms[4 * (A_DXDX)] = dxdx;
    terms[4 * (A_DXDY)] = dxdy;
    terms[4 * (A_DYDY)] = dydy;
    terms[4 * (A_B0 + 0)] = -(dt * x * dx);
    terms[4 * (A_B0 + 1)] = -(dt * x * dy);
    terms[4 * (A_B0 + 2)] = -(dt * y * dx);
    terms[4 * (A_B0 + 3)] = -(dt * y * dy);
    terms[4 * (A_B0 + 4)] = -(dt * dx);
    terms[4 * (A_B0 + 5)] = -(dt * dy);
}

__device__ __forceinline__ void affine_fill_matrix(const float *sums, float (&m)[6][6]) {
    const float h00 = sums[A_XX_DXDX], h01 = sums[A_XX_DXDY], h02 = sums[A_XY_DXDX], h03 = sums[A_XY_DXDY];
    const float h04 = sums[A_X_DXDX], h05 = sums[A_X_DXDY], h11 = sums[A_XX_DYDY], h13 = sums[A_XY_DYDY];
    const float h15 = sums[A_X_DYDY], h22 = sums[A_YY_DXDX], h23 = sums[A_YY_DXDY], h24 = sums[A_Y_DXDX];
    const float h25 = sums[A_Y_DXDY], h33 = sums[A_YY_DYDY], h35 = sums[A_Y_DYDY], h44 = sums[A_DXDX];
    const float h45 = sums[A_DXDY], h55 = sums[A_DYDY];
    const float h12 = h03, h14 = h05, h34 = h23;
    const float u[6][6] = {{h00, h01, h02, h03, h04, h05}, {h01, h11, h12, h13, h14, h15}, {h02, h12, h22, h23, h24, h25},
                           {h03, h13, h23, h33, h34, h35}, {h04, h14, h24, h34, h44, h45}, {h05, h15, h25, h35, h45, h55}};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            m[i][j] = u[i][j];
        }
    }
}

__device__ __forceinline__ void affine_apply_step(AffineState &s, const float (&z)[6], const float (&v)[2]) {
    s.cur_u += v[0];
    s.cur_v += v[1];
    s.a00 += z[0];
    s.a10 += z[1];
    s.a01 += z[2];
    s.a11 += z[3];
}

// TrackOneFeature, affine_klt.cpp:93-273.
//
// Work split of one iteration when the patch has more pixels than the workgroup has lanes (W = 2 at 13 x 13: 169 > 128): all waves
// produce the products of the first 64 W pixels together; then wave 0 starts the exact-order chains on those while the other
// waves produce the remaining pixels, and continues over the rest after one more barrier — the chain (the iteration's longest
// dependent stretch) no longer waits for a second, mostly empty, round of sampling.  Same products, same row-major order.
template <int METHOD>
__device__ __forceinline__ void affine_level(const Blk &b, const KltParams &p, const DevImage &ref, const DevImage &cur, float ref_u, float ref_v,
                                             AffineState &s, uint8_t &status, uint32_t &iters, Carve &c) {
    Win rw, cw;
    stage_level_windows(b, p, ref, cur, ref_u, ref_v, s.cur_u, s.cur_v, c, rw, cw, (METHOD == FTK_METHOD_INVERSE) ? 3 : 1);
    bool cw_staged = true;
    nonfast_level_setup<METHOD, true>(b, p, ref, rw, ref_u, ref_v, c);
    const bool staged = !b.solo && b.nwaves > 1 && p.P > b.nt;
    const uint32_t dense_slots = affine_dense_slots(b.lane);  // chain lane -> its entries of the dense Hessian (wave 0)
    for (uint32_t iter = 0; iter < p.max_iteration; ++iter) {
        ++iters;
        ensure_cur_window(b, p, cur, s.cur_u, s.cur_v, c, cw, cw_staged);
        bool miss_unused = false;
        // the 24 products of one patch pixel -> terms[k][pxi]; returns whether the pixel is used
        auto produce = [&](int pxi) -> bool {
            int prow, pcol;
            pixel_rc(p, pxi, prow, pcol);
            const float dcol = (float)(pcol - p.half_cols);
            const float drow = (float)(prow - p.half_rows);
            const float warped_x = s.a00 * dcol + s.a01 * drow;
            const float warped_y = s.a10 * dcol + s.a11 * drow;
            const float row_j = warped_y + s.cur_v;
            const float col_j = warped_x + s.cur_u;
            float dx, dy, i_ref, i_cur;
            const bool ok = nonfast_gather<METHOD, kGatherInline, true>(cur, cw, c, pxi, row_j, col_j, dx, dy, i_ref, i_cur, miss_unused);
            const float dt = i_cur - i_ref;
            affine_all_terms(c.terms, pxi, ok, dt, col_j, row_j, dx, dy);
            return ok;
        };
        uint32_t n_valid = 0;
        float acc = 0.0f;
        if (!staged) {
            for (int base = 0; base < p.P; base += b.nt) {
                const int pxi = base + b.tid;
                const bool ok = pxi < p.P ? produce(pxi) : false;
                n_valid += (uint32_t)__popcll(wave_ballot(ok));
            }
            publish_count(b, n_valid, c.wave_cnt, iter);
            blk_sync(b);  // the terms (and the published counts) are visible
            // (The 24 sums as quad chains on TWO waves side by side — 16 + 8 quads, published through LDS, one more barrier — were built
            // and measured in round 5: slower, config 3 139.8 -> 149.1 us, real pair 300 features 89.1 -> 91.1; docs/LAB_NOTES.md.)
            if (b.wave == 0 && b.lane < A_COUNT) {
                acc = chain_groups<kAffineGroup / 4>(reinterpret_cast<const float4 *>(c.terms) + b.lane, affine_group_rounds(p.Ppad), 0.0f);
            }
        } else {
            {
                const bool ok = produce(b.tid);  // P > nt: every lane has a pixel
                n_valid += (uint32_t)__popcll(wave_ballot(ok));
            }
            blk_sync(b);  // the products of pixels [0, nt) are visible
            if (b.wave == 0) {
                if (b.lane < A_COUNT) {
                    acc = chain_groups<kAffineGroup / 4>(reinterpret_cast<const float4 *>(c.terms) + b.lane, b.nt / (4 * kChainRound), 0.0f);
                }
            } else {
                const int step = b.nt - kWave;
                for (int base = b.nt; base < p.P; base += step) {
                    const int pxi = base + (b.tid - kWave);
                    const bool ok = pxi < p.P ? produce(pxi) : false;
                    n_valid += (uint32_t)__popcll(wave_ballot(ok));
                }
            }
            publish_count(b, n_valid, c.wave_cnt, iter);
            blk_sync(b);  // the remaining products and every wave's count are visible
            if (b.wave == 0 && b.lane < A_COUNT) {
                acc = chain_groups<kAffineGroup / 4>(reinterpret_cast<const float4 *>(c.terms) + (b.nt >> 2) * (kAffineGroup / 4) + b.lane,
                                                     affine_group_rounds(p.Ppad) - b.nt / (4 * kChainRound), acc);
            }
        }
        if (b.wave == 0) {
            // The chain lanes publish their sums as the DENSE row-major Hessian (sums[32..68), every alias written by the lane that
            // owns the sum) and the six bias sums; the diagonal the pivot search needs is read from the accumulators themselves.
            float *const dense = c.sums + 32;
            if (b.lane < 18) {
                dense[dense_slots & 0xffu] = acc;
                dense[(dense_slots >> 8) & 0xffu] = acc;
                dense[(dense_slots >> 16) & 0xffu] = acc;
                dense[dense_slots >> 24] = acc;
            } else if (b.lane < A_COUNT) {
                c.sums[b.lane] = acc;
            }
            float ad_all[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                ad_all[j] = fabsf(bcast_lane(acc, kAffineDiagLane[j]));
            }
            float my_ad = ad_all[0];
#pragma unroll
            for (int j = 1; j < 6; ++j) {
                my_ad = (b.lane == j) ? ad_all[j] : my_ad;
            }
            __builtin_amdgcn_wave_barrier();  // same-wave LDS traffic is ordered
            const Ldlt6 fac = ldlt6_factor_diag(my_ad, ad_all, Ldlt6Dense{dense}, b.lane);
            ldlt6_solve(fac, c.sums + A_B0, c.sums + A_COUNT, b.lane);
            // every wave's count was published before the barrier in front of the last chain segment: their total travels with
            // the solution, so that the waves read both with one LDS round trip after the barrier below
            if (b.lane == 0) {
                reinterpret_cast<uint32_t *>(c.sums)[A_COUNT + 6] = collect_count(b, c.wave_cnt, iter);
            }
        }
        blk_sync(b);  // the solution is visible
        n_valid = reinterpret_cast<const uint32_t *>(c.sums)[A_COUNT + 6];
        const float z[6] = {c.sums[A_COUNT], c.sums[A_COUNT + 1], c.sums[A_COUNT + 2], c.sums[A_COUNT + 3], c.sums[A_COUNT + 4], c.sums[A_COUNT + 5]};
        if (n_valid == 0) {
            break;
        }
        float v[2];
        v[0] = (z[0] * s.cur_u + z[2] * s.cur_v) + z[4];
        v[1] = (z[1] * s.cur_u + z[3] * s.cur_v) + z[5];
        if (isnan(v[0]) || isnan(v[1])) {
            status = FTK_NUMERIC_ERROR;
            break;
        }
        affine_apply_step(s, z, v);
        if (uv_outside(s.cur_u, s.cur_v, cur)) {
            status = FTK_OUTSIDE;
            break;
        }
        if (v[0] * v[0] + v[1] * v[1] < p.converge) {
            status = FTK_TRACKED;
            break;
        }
    }
}

// TrackOneFeatureFast, affine_klt_fast.cpp:7-188.
__device__ __forceinline__ void affine_level_fast(const Blk &b, const KltParams &p, const DevImage &ref, const DevImage &cur, float ref_u,
                                                  float ref_v, AffineState &s, uint8_t &status, uint32_t &iters, Carve &c) {
    float *ex = c.a0, *dxs = c.a1, *dys = c.a2;
    uint8_t *exv = c.flagsE;
    Win rw, cw;
    stage_level_windows(b, p, ref, cur, ref_u, ref_v, s.cur_u, s.cur_v, c, rw, cw);
    bool cw_staged = true;
    if (extract_extended_patch(b, p, ref, rw, ref_u, ref_v, c) == 0) {
        status = FTK_OUTSIDE;
        return;
    }
    // H once per level, anchored at cur_uv on level entry (:95-96)
    for (int pxi = b.tid; pxi < p.P; pxi += b.nt) {
        int prow, pcol;
        pixel_rc(p, pxi, prow, pcol);
        float dx, dy;
        const bool has_gradient = ex_gradient(p, ex, exv, prow, pcol, dx, dy);
        dxs[pxi] = dx;
        dys[pxi] = dy;
        const float x = (float)(pcol - p.half_cols) + s.cur_u;
        const float y = (float)(prow - p.half_rows) + s.cur_v;
        affine_hessian_terms(p, c.terms, pxi, has_gradient, x, y, dx, dy);
    }
    blk_sync(b);
    // The Hessian is fixed for the level (affine_klt_fast.cpp:71-138), so it is FACTORISED once here — rows on
    // lanes 0..5 of wave 0 — and every iteration below only runs the two triangular solves (same arithmetic as
    // factorising each time: the factorisation is a pure function of H).
    Ldlt6 fac;
    fac.perm = 0;
    fac.d_mine = 0.0f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        fac.l[i] = 0.0f;
    }
    chain_then(b, c.terms, A_B0, p.Ppad, c.sums, false, [&]() {
        float h[6][6];
        affine_fill_matrix(c.sums, h);
        if (b.lane == 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    c.sums[32 + i * 6 + j] = h[i][j];
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        fac = ldlt6_factor(c.sums + 32, b.lane);
    });

    status = FTK_LARGE_RESIDUAL;
    float last_squared_step = INFINITY;
    uint32_t large_step_cnt = 0;
    for (uint32_t iter = 0; iter < p.max_iteration; ++iter) {
        ++iters;
        ensure_cur_window(b, p, cur, s.cur_u, s.cur_v, c, cw, cw_staged);
        uint32_t n_valid = 0;
        for (int base = 0; base < p.P; base += b.nt) {
            const int pxi = base + b.tid;
            bool ok = false;
            if (pxi < p.P) {
                int prow, pcol;
                pixel_rc(p, pxi, prow, pcol);
                const float dcol = (float)(pcol - p.half_cols);
                const float drow = (float)(prow - p.half_rows);
                const float warped_x = s.a00 * dcol + s.a01 * drow;
                const float warped_y = s.a10 * dcol + s.a11 * drow;
                const float row_c = warped_y + s.cur_v;
                const float col_c = warped_x + s.cur_u;
                float i_cur = 0.0f;
                const int ei = imul(prow + 1, p.ex_cols) + pcol + 1;
                ok = sample(cur, cw, row_c, col_c, i_cur) && exv[ei] != 0;
                const float dt = i_cur - ex[ei];
                affine_bias_terms(p, c.terms, 0, pxi, ok, dt, col_c, row_c, dxs[pxi], dys[pxi]);
            }
            n_valid += (uint32_t)__popcll(wave_ballot(ok));
        }
        publish_count(b, n_valid, c.wave_cnt, iter);
        chain_then(b, c.terms, 6, p.Ppad, c.sums, true, [&]() {
            ldlt6_solve(fac, c.sums, c.sums + A_COUNT, b.lane);
            if (b.lane == 0) {
                reinterpret_cast<uint32_t *>(c.sums)[A_COUNT + 6] = collect_count(b, c.wave_cnt, iter);  // travels with the solution
            }
        });
        n_valid = reinterpret_cast<const uint32_t *>(c.sums)[A_COUNT + 6];
        const float z[6] = {c.sums[A_COUNT], c.sums[A_COUNT + 1], c.sums[A_COUNT + 2], c.sums[A_COUNT + 3], c.sums[A_COUNT + 4], c.sums[A_COUNT + 5]};
        if (n_valid == 0) {
            break;
        }
        if (isnan(z[0]) || isnan(z[1]) || isnan(z[2]) || isnan(z[3]) || isnan(z[4]) || isnan(z[5])) {
            status = FTK_NUMERIC_ERROR;
            break;
        }
        float v[2];
        v[0] = (z[0] * s.cur_u + z[2] * s.cur_v) + z[4];
        v[1] = (z[1] * s.cur_u + z[3] * s.cur_v) + z[5];
        affine_apply_step(s, z, v);
        if (fast_step_logic(p, v[0] * v[0] + v[1] * v[1], last_squared_step, large_step_cnt, status)) {
            break;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// LSSD KLT (SE(2), 3x3).  Chains: 0 j0j0, 1 j0j1, 2 j0j2, 3 j1j1, 4 j1j2, 5 j2j2, 6..8 -j_i*r.
// ---------------------------------------------------------------------------------------------
struct LssdState {
    float r00, r01, r10, r11;
    float t0, t1;
};

__device__ __forceinline__ void se2_apply(const LssdState &s, float x, float y, float &ox, float &oy) {
    ox = (s.r00 * x + s.r01 * y) + s.t0;
    oy = (s.r10 * x + s.r11 * y) + s.t1;
}

// delta_R << 1, -theta, theta, 1; R *= delta_R; R /= R.col(0).norm(); t += v.tail<2>()
// kLanes (one-wave trackers: wave-uniform state, all lanes executing): the four divisions by the norm run on four lanes.
template <bool kLanes = false>
__device__ __forceinline__ void se2_update(LssdState &s, const float (&v)[3], int lane = 0) {
    const float theta = v[0];
    const float d00 = 1.0f, d01 = -theta, d10 = theta, d11 = 1.0f;
    const float n00 = s.r00 * d00 + s.r01 * d10;
    const float n01 = s.r00 * d01 + s.r01 * d11;
    const float n10 = s.r10 * d00 + s.r11 * d10;
    const float n11 = s.r10 * d01 + s.r11 * d11;
    const float norm = sqrtf(n00 * n00 + n10 * n10);
    if (kLanes) {
        const float q = (lane == 0 ? n00 : (lane == 1 ? n01 : (lane == 2 ? n10 : n11))) / norm;
        s.r00 = bcast_lane(q, 0);
        s.r01 = bcast_lane(q, 1);
        s.r10 = bcast_lane(q, 2);
        s.r11 = bcast_lane(q, 3);
    } else {
        s.r00 = n00 / norm;
        s.r01 = n01 / norm;
        s.r10 = n10 / norm;
        s.r11 = n11 / norm;
    }
    s.t0 += v[1];
    s.t1 += v[2];
}

// Vec3::squaredNorm(): Eigen's unrolled reduction of a fixed 3-vector is a0 + (a1 + a2)
__device__ __forceinline__ float vec3_squared_norm(const float (&v)[3]) { return v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]); }

// The nine products of a pixel, in the order of the chains (the header of this section) — the ONE place that states them: the
// upper triangle of J^T J row by row for J = (j0, j1, j2), then -J^T r.  `put(k, product)` stores product k where its caller sums.
template <typename Put>
__device__ __forceinline__ void lssd_products(float j0, float j1, float j2, float residual, Put put) {
    put(0, j0 * j0);
    put(1, j0 * j1);
    put(2, j0 * j2);
    put(3, j1 * j1);
    put(4, j1 * j2);
    put(5, j2 * j2);
    put(6, -(j0 * residual));
    put(7, -(j1 * residual));
    put(8, -(j2 * residual));
}

__device__ __forceinline__ void lssd_terms(const KltParams &p, float *terms, int pxi, bool ok, float j0, float j1, float j2, float residual) {
    lssd_products(j0, j1, j2, residual, [&](int k, float product) { terms[k * p.Ppad + pxi] = ok ? product : 0.0f; });
}

// Wave 0: solves the 3x3 system from the nine chain sums and publishes v in sums[16..18].
__device__ __forceinline__ void lssd_solve(float *sums, int lane) {
    const float h00 = sums[0], h01 = sums[1], h02 = sums[2], h11 = sums[3], h12 = sums[4], h22 = sums[5];
    const float bb[3] = {sums[6], sums[7], sums[8]};
    float sol[3];
    ldlt3_solve<true>(h00, h01, h02, h11, h12, h22, bb, sol, lane);  // the whole of wave 0 is here, on the same sums
    sums[16] = sol[0];
    sums[17] = sol[1];
    sums[18] = sol[2];
}

// Every lane: picks up the published solution and applies the SE(2) update.
// Returns false (after setting status) on NaN.
__device__ __forceinline__ bool lssd_solve_and_update(const float *sums, LssdState &s, float (&v)[3], uint8_t &status, int lane) {
    v[0] = sums[16];
    v[1] = sums[17];
    v[2] = sums[18];
    if (isnan(v[0]) || isnan(v[1]) || isnan(v[2])) {
        status = FTK_NUMERIC_ERROR;
        return false;
    }
    se2_update<true>(s, v, lane);  // every wave in full, on the same published solution
    return true;
}

// --- per-pixel helpers of the three LSSD-fast level forms (lssd_level_fast, lssd_level_fast_chunked, lssd_level_fast_chunked_lum) ---

// ExtractPatchInCurrentImage's test (lssd_klt_fast.cpp:145-160): does the conservative bounding box of the patch around `centre`
// leave the rectangle in which every bilinear tap is inside `cur`?  Wave-uniform: scalar from the readfirstlane on.
__device__ __forceinline__ bool lssd_partly_outside(const KltParams &p, const DevImage &cur, float centre_u, float centre_v) {
    const int min_row = wadd(__builtin_amdgcn_readfirstlane(f2i(centre_v)), -p.patch_rows);
    const int min_col = wadd(__builtin_amdgcn_readfirstlane(f2i(centre_u)), -p.patch_cols);
    const int max_row = wadd(min_row, p.patch_rows * 2);
    const int max_col = wadd(min_col, p.patch_cols * 2);
    return min_row < 0 || max_row > cur.rows - 2 || min_col < 0 || max_col > cur.cols - 2;
}

// One pixel of the current patch (lssd_klt_fast.cpp:162-193): the checked sample with a zeroed miss when the patch is partly
// outside, the unchecked bilinear (:189) otherwise.
// kRoomy (the one-wave chunked forms; every lane of the wave must be here): when every lane's sample lies inside the image with
// room for its +1 neighbours (the normal case: a rotation moves a pixel less than the conservative box of lssd_partly_outside
// allows for) the cheaper bilinear_inside gives the same values.
template <bool kRoomy>
__device__ __forceinline__ bool lssd_sample_cur(const DevImage &cur, const Win &cw, float row_j, float col_j, bool partly_outside, float &value) {
    bool ok_cur;
    value = 0.0f;
    if (partly_outside) {
        ok_cur = sample(cur, cw, row_j, col_j, value);
        if (!ok_cur) {
            value = 0.0f;
        }
    } else {
        bool all_roomy = false;
        if constexpr (kRoomy) {
            // 0 <= x <= M as ONE unsigned compare of the bit patterns (M >= 0 here: !partly_outside): negative values, -0 and
            // NaNs have larger patterns than any finite M and take the general form below, which returns the same values
            const bool roomy = (unsigned)__float_as_int(row_j) <= (unsigned)__float_as_int((float)(cur.rows - 2)) &&
                               (unsigned)__float_as_int(col_j) <= (unsigned)__float_as_int((float)(cur.cols - 2));
            all_roomy = wave_ballot(!roomy) == 0ull;
        }
        if (all_roomy) {
            value = bilinear_inside(cur, cw, row_j, col_j);
        } else {
            value = bilinear(cur, cw, row_j, col_j);
        }
        ok_cur = true;
    }
    return ok_cur;
}

// The Jacobian's rotation column of the pixel at (row_i, col_i) with gradient (dx, dy) (lssd_klt_fast.cpp:214-219); the other two
// columns are dx and dy themselves.
__device__ __forceinline__ float lssd_pixel_j0(const LssdState &s, float row_i, float col_i, float dx, float dy) {
    const float s0 = s.r00 * (-row_i) + s.r01 * col_i;
    const float s1 = s.r10 * (-row_i) + s.r11 * col_i;
    return dx * s0 + dy * s1;
}

// A lane's pixel of a chunk into the ring ([9][kChunkRow]): its nine products (lssd_products), row k = product k.  `px` is the
// pixel's record {dx, dy, reference value, valid} (lssd_chunked_entry), `value` its sample in the current image.
// An unused pixel contributes exact zeros to every sum (lssd_terms): zeroing the four factors does it with four selects instead of
// nine — the products are then +0 or -0, and x + (+-0) == x for every x a sum can hold (the sums start at +0 and +0 + (-0) == +0).
__device__ __forceinline__ void lssd_ring_products(float *ring, int lane, bool ok, const LssdState &s, float row_i, float col_i, const float4 &px,
                                                   float value) {
    const float dx = ok ? px.x : 0.0f, dy = ok ? px.y : 0.0f;
    const float j0 = ok ? lssd_pixel_j0(s, row_i, col_i, px.x, px.y) : 0.0f;
    const float residual = ok ? value - px.z : 0.0f;
    lssd_products(j0, dx, dy, residual, [&](int k, float product) { ring[k * kChunkRow + lane] = product; });
}

// Advances the kSums exact-order sums (9: the products; 1: the luminance form's mean, in ring row 0) over chunk `chunk` of the ring.
// quad chain: every lane works, quad q carries sum q (klt_chain.h "quad chain"); the quads behind the last sum follow its row and
// are ignored.  A launch that oversubscribes the chip keeps one lane per sum (KltParams::quad_chain): there the instruction COUNT
// decides.  Either way sum k ends in lane k * sum_lanes(p).
template <int kSums>
__device__ __forceinline__ float lssd_chain_ring(const Blk &b, const KltParams &p, const float *ring, int chunk, float acc) {
    const int left = p.P - chunk * kChunkPixels;
    if (p.quad_chain) {
        return chain_quads_left(acc, ring + min(b.lane >> 2, kSums - 1) * kChunkRow + 4 * (b.lane & 3), left);
    }
    if (b.lane < kSums) {
        return chain_chunk_left(acc, ring + b.lane * kChunkRow, left);
    }
    return acc;
}

// What a chunked level keeps from its entry (lssd_chunked_entry) to its iterations.
struct LssdChunked {
    float *ring;        // [9][kChunkRow]
    const float4 *rec;  // per patch pixel: {dx, dy, reference value, valid}
    const float2 *rc;   // per patch pixel: {row_i, col_i}
    int n_chunks;
    Win cw;
    bool cw_staged;
    float last_squared_step;
    uint32_t large_step_cnt;
};

// The tail of a chunked iteration: the nine sums sit in `acc` of lanes k * sum_lanes(p) — broadcast (v_readlane, no round trip
// through LDS), solve (lssd_solve on registers), update `s`.  Returns whether the level goes on; `status` is set when it does not.
__device__ __forceinline__ bool lssd_chunked_step(const Blk &b, const KltParams &p, float acc, LssdState &s, LssdChunked &lv, uint8_t &status) {
    const int acc_bits = __float_as_int(acc);
    const int sl = __builtin_amdgcn_readfirstlane(sum_lanes(p));
    float sum[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        sum[k] = __int_as_float(__builtin_amdgcn_readlane(acc_bits, k * sl));
    }
    const float bb[3] = {sum[6], sum[7], sum[8]};
    float v[3];
    ldlt3_solve<true>(sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], bb, v, b.lane);
    if (isnan(v[0]) || isnan(v[1]) || isnan(v[2])) {
        status = FTK_NUMERIC_ERROR;
        return false;
    }
    se2_update<true>(s, v, b.lane);
    return !fast_step_logic(p, vec3_squared_norm(v), lv.last_squared_step, lv.large_step_cnt, status);
}

// The level entry of the two chunked forms (lssd_klt_fast.cpp:7-46).  Returns false (status = FTK_OUTSIDE) when no pixel of the
// extended reference patch is inside the image.
// The chunked variants have a0_floats == 0: the extended patch (level entry only) lives in the ring's space (iterations only).
// What an iteration needs of a patch pixel is laid out by pixel: {dx, dy, reference value, valid} and {row_i, col_i} — one
// 16-byte and one 8-byte conflict-free read per pixel instead of the row / column division, the index into the extended
// patch and four scattered reads, every iteration.
// LUM (consider_patch_luminance, :27-46): the gradients and the patch value are each divided by the reference mean (the gradients
// are differences of UNSCALED values).  The reference's quirk is kept: the mean's numerator covers the interior of the EXTENDED
// patch (= the patch) and its denominator the valid count of the whole extended patch.
template <bool LUM>
__device__ __forceinline__ bool lssd_chunked_entry(const Blk &b, const KltParams &p, const DevImage &ref, const DevImage &cur, float ref_u,
                                                   float ref_v, const LssdState &s, uint8_t &status, Carve &c, LssdChunked &lv) {
    c.a0 = c.terms;
    const float *ex = c.a0;
    const uint8_t *exv = c.flagsE;
    float4 *rec = reinterpret_cast<float4 *>(c.a1);
    float2 *rc = reinterpret_cast<float2 *>(c.a1 + 4 * p.Ppad);
    lv.ring = c.terms;
    lv.rec = rec;
    lv.rc = rc;
    lv.n_chunks = (p.P + kChunkPixels - 1) / kChunkPixels;
    Win rw;
    float level_centre_u, level_centre_v;
    se2_apply(s, ref_u, ref_v, level_centre_u, level_centre_v);
    stage_level_windows(b, p, ref, cur, ref_u, ref_v, level_centre_u, level_centre_v, c, rw, lv.cw);
    lv.cw_staged = true;
    const uint32_t ref_valid_num = extract_extended_patch(b, p, ref, rw, ref_u, ref_v, c);
    if (ref_valid_num == 0) {
        status = FTK_OUTSIDE;
        return false;
    }
    float ref_average = 1.0f;
    if constexpr (LUM) {
        // :27-35 — the interior of the extended patch in row-major order (== the P patch pixels), summed by lane 0 from a
        // contiguous row laid over the (not yet written) per-pixel records
        float *row = c.a1;
        for (int pxi = b.tid; pxi < p.Ppad; pxi += b.nt) {
            int prow, pcol;
            pixel_rc(p, pxi < p.P ? pxi : 0, prow, pcol);
            row[pxi] = pxi < p.P ? ex[imul(prow + 1, p.ex_cols) + pcol + 1] : 0.0f;
        }
        blk_sync(b);
        float ref_sum = 0.0f;
        if (b.lane == 0) {
            ref_sum = chain_lane(row, p.Ppad);
        }
        ref_average = bcast_lane(ref_sum, 0) / (float)ref_valid_num;
        blk_sync(b);
    }
    for (int pxi = b.tid; pxi < p.P; pxi += b.nt) {
        int prow, pcol;
        pixel_rc(p, pxi, prow, pcol);
        float dx, dy;
        ex_gradient(p, ex, exv, prow, pcol, dx, dy);
        const int ei = imul(prow, p.ex_cols) + pcol + (p.ex_cols + 1);
        float value = ex[ei];
        if constexpr (LUM) {
            dx /= ref_average;
            dy /= ref_average;
            value /= ref_average;
        }
        rec[pxi] = make_float4(dx, dy, value, __int_as_float(exv[ei] != 0 ? -1 : 0));
        rc[pxi] = make_float2((float)(prow - p.half_rows) + ref_v, (float)(pcol - p.half_cols) + ref_u);
    }
    blk_sync(b);
    status = FTK_LARGE_RESIDUAL;
    lv.last_squared_step = INFINITY;
    lv.large_step_cnt = 0;
    return true;
}

// TrackOneFeature, lssd_klt.cpp:96-250.  a0 = i_cur of the current iteration.
template <int METHOD>
__device__ __forceinline__ void lssd_level(const Blk &b, const KltParams &p, const DevImage &ref, const DevImage &cur, float ref_u, float ref_v,
                                           LssdState &s, uint8_t &status, uint32_t &iters, Carve &c) {
    Win rw, cw;
    float level_centre_u, level_centre_v;
    se2_apply(s, ref_u, ref_v, level_centre_u, level_centre_v);
    stage_level_windows(b, p, ref, cur, ref_u, ref_v, level_centre_u, level_centre_v, c, rw, cw, (METHOD == FTK_METHOD_INVERSE) ? 3 : 1);
    bool cw_staged = true;
    nonfast_level_setup<METHOD>(b, p, ref, rw, ref_u, ref_v, c);
    uint8_t *okflags = c.flagsE;  // per-iteration validity of a pixel (all six fetches)
    float *icur = c.a0;
    for (uint32_t iter = 0; iter < p.max_iteration; ++iter) {
        ++iters;
        float centre_u, centre_v;
        se2_apply(s, ref_u, ref_v, centre_u, centre_v);
        ensure_cur_window(b, p, cur, centre_u, centre_v, c, cw, cw_staged);
        // pass 1 (:140-184): validity mask and the two patch means (sequential sums)
        uint32_t n_valid = 0;
        bool miss_unused = false;
        for (int base = 0; base < p.P; base += b.nt) {
            const int pxi = base + b.tid;
            bool ok = false;
            if (pxi < p.P) {
                int prow, pcol;
                pixel_rc(p, pxi, prow, pcol);
                const float row_i = (float)(prow - p.half_rows) + ref_v;
                const float col_i = (float)(pcol - p.half_cols) + ref_u;
                float row_j, col_j;
                se2_apply(s, col_i, row_i, col_j, row_j);
                float gx, gy, i_ref, i_cur;
                ok = nonfast_gather<METHOD, kGatherInline>(cur, cw, c, pxi, row_j, col_j, gx, gy, i_ref, i_cur, miss_unused);
                if (METHOD != FTK_METHOD_INVERSE) {
                    c.a1[pxi] = gx;
                    c.a2[pxi] = gy;
                }
                icur[pxi] = i_cur;
                okflags[pxi] = ok ? 1 : 0;
                c.terms[0 * p.Ppad + pxi] = ok ? i_ref : 0.0f;
                c.terms[1 * p.Ppad + pxi] = ok ? i_cur : 0.0f;
            }
            n_valid += (uint32_t)__popcll(wave_ballot(ok));
        }
        n_valid = block_total(b, n_valid, c.wave_cnt);
        chain_sums(b, c.terms, 2, p.Ppad, c.sums);
        const float ref_average = c.sums[0] / (float)n_valid;
        const float cur_average = c.sums[1] / (float)n_valid;
        const float grad_average = (METHOD == FTK_METHOD_INVERSE) ? ref_average : cur_average;
        blk_sync(b);  // sums[] is rewritten by the second chain below

        // pass 2 (:186-247): mean-normalised Jacobian and residual
        for (int pxi = b.tid; pxi < p.P; pxi += b.nt) {
            int prow, pcol;
            pixel_rc(p, pxi, prow, pcol);
            const float row_i = (float)(prow - p.half_rows) + ref_v;
            const float col_i = (float)(pcol - p.half_cols) + ref_u;
            const bool ok = okflags[pxi] != 0;
            const float jp0 = c.a1[pxi] / grad_average;
            const float jp1 = c.a2[pxi] / grad_average;
            const float s0 = s.r00 * (-row_i) + s.r01 * col_i;
            const float s1 = s.r10 * (-row_i) + s.r11 * col_i;
            const float j0 = jp0 * s0 + jp1 * s1;
            const float j1 = jp0 * 1.0f + jp1 * 0.0f;
            const float j2 = jp0 * 0.0f + jp1 * 1.0f;
            const float residual = icur[pxi] / cur_average - c.a3[pxi] / ref_average;
            lssd_terms(p, c.terms, pxi, ok, j0, j1, j2, residual);
        }
        blk_sync(b);
        if (n_valid == 0) {
            break;
        }
        chain_then(b, c.terms, 9, p.Ppad, c.sums, false, [&]() { lssd_solve(c.sums, b.lane); });
        float v[3];
        const bool solved = lssd_solve_and_update(c.sums, s, v, status, b.lane);
        blk_sync(b);  // sums[] is rewritten by the first chain of the next iteration
        if (!solved) {
            break;
        }
        if (vec3_squared_norm(v) < p.converge) {
            status = FTK_TRACKED;
            break;
        }
    }
}

// TrackOneFeatureFast, lssd_klt_fast.cpp:7-229.  a3 = current patch, flagsP = its validity.
__device__ __forceinline__ void lssd_level_fast(const Blk &b, const KltParams &p, const DevImage &ref, const DevImage &cur, float ref_u,
                                                float ref_v, LssdState &s, uint8_t &status, uint32_t &iters, Carve &c) {
    float *ex = c.a0, *dxs = c.a1, *dys = c.a2, *curp = c.a3;
    uint8_t *exv = c.flagsE, *curv = c.flagsP;
    Win rw, cw;
    float level_centre_u, level_centre_v;
    se2_apply(s, ref_u, ref_v, level_centre_u, level_centre_v);
    stage_level_windows(b, p, ref, cur, ref_u, ref_v, level_centre_u, level_centre_v, c, rw, cw);
    bool cw_staged = true;
    const uint32_t ref_valid_num = extract_extended_patch(b, p, ref, rw, ref_u, ref_v, c);
    if (ref_valid_num == 0) {
        status = FTK_OUTSIDE;
        return;
    }
    for (int pxi = b.tid; pxi < p.P; pxi += b.nt) {
        int prow, pcol;
        pixel_rc(p, pxi, prow, pcol);
        float dx, dy;
        ex_gradient(p, ex, exv, prow, pcol, dx, dy);
        dxs[pxi] = dx;
        dys[pxi] = dy;
        // interior of the extended patch in row-major order == the P patch pixels
        c.terms[pxi] = ex[imul(prow + 1, p.ex_cols) + pcol + 1];
    }
    blk_sync(b);
    if (p.consider_luminance) {
        // :27-46 — numerator: interior of the extended patch; denominator: valid count of the WHOLE extended patch
        chain_sums(b, c.terms, 1, p.Ppad, c.sums);
        const float ref_average = c.sums[0] / (float)ref_valid_num;
        for (int i = b.tid; i < p.P; i += b.nt) {
            dxs[i] /= ref_average;
            dys[i] /= ref_average;
        }
        for (int i = b.tid; i < p.E; i += b.nt) {
            ex[i] /= ref_average;
        }
        blk_sync(b);
    }

    status = FTK_LARGE_RESIDUAL;
    float last_squared_step = INFINITY;
    uint32_t large_step_cnt = 0;
    for (uint32_t iter = 0; iter < p.max_iteration; ++iter) {
        ++iters;
        // ExtractPatchInCurrentImage (:145-195)
        float centre_u, centre_v;
        se2_apply(s, ref_u, ref_v, centre_u, centre_v);
        ensure_cur_window(b, p, cur, centre_u, centre_v, c, cw, cw_staged);
        const bool partly_outside = lssd_partly_outside(p, cur, centre_u, centre_v);
        uint32_t cur_valid_num = 0;
        if (!p.consider_luminance) {
            // Without the luminance scaling nothing separates ExtractPatchInCurrentImage from ComputeHessianAndBias but
            // the "no valid pixel" exits, so one sweep samples a pixel and forms its nine products right away (same
            // expressions, same values; the patch never makes the round trip through LDS).
            uint32_t n_valid = 0;
            for (int base = 0; base < p.P; base += b.nt) {
                const int pxi = base + b.tid;
                bool ok_cur = false, ok = false;
                if (pxi < p.P) {
                    int prow, pcol;
                    pixel_rc(p, pxi, prow, pcol);
                    const float row_i = (float)(prow - p.half_rows) + ref_v;
                    const float col_i = (float)(pcol - p.half_cols) + ref_u;
                    float row_j, col_j;
                    se2_apply(s, col_i, row_i, col_j, row_j);
                    float value;
                    ok_cur = lssd_sample_cur<false>(cur, cw, row_j, col_j, partly_outside, value);
                    const int ei = imul(prow + 1, p.ex_cols) + pcol + 1;
                    ok = exv[ei] != 0 && ok_cur;
                    const float dx = dxs[pxi], dy = dys[pxi];
                    lssd_terms(p, c.terms, pxi, ok, lssd_pixel_j0(s, row_i, col_i, dx, dy), dx, dy, value - ex[ei]);
                }
                cur_valid_num += (uint32_t)__popcll(wave_ballot(ok_cur));
                n_valid += (uint32_t)__popcll(wave_ballot(ok));
            }
            // both counts in one exchange: n_valid <= cur_valid_num <= P < 2^16
            const uint32_t both = block_total(b, (cur_valid_num << 16) | n_valid, c.wave_cnt);
            if ((both >> 16) == 0 || (both & 0xFFFFu) == 0) {
                break;  // lssd_klt_fast.cpp:60-63 / :80-83
            }
            chain_then(b, c.terms, 9, p.Ppad, c.sums, false, [&]() { lssd_solve(c.sums, b.lane); });
            float v[3];
            const bool solved = lssd_solve_and_update(c.sums, s, v, status, b.lane);
            blk_sync(b);
            if (!solved) {
                break;
            }
            if (fast_step_logic(p, vec3_squared_norm(v), last_squared_step, large_step_cnt, status)) {
                break;
            }
            continue;
        }
        for (int base = 0; base < p.P; base += b.nt) {
            const int pxi = base + b.tid;
            bool ok = false;
            if (pxi < p.P) {
                int prow, pcol;
                pixel_rc(p, pxi, prow, pcol);
                const float row_i = (float)(prow - p.half_rows) + ref_v;
                const float col_i = (float)(pcol - p.half_cols) + ref_u;
                float row_j, col_j;
                se2_apply(s, col_i, row_i, col_j, row_j);
                float value;
                ok = lssd_sample_cur<false>(cur, cw, row_j, col_j, partly_outside, value);
                curp[pxi] = value;
                curv[pxi] = ok ? 1 : 0;
                // :65-71 — the mean numerator only covers patch rows / cols 1 .. size-2
                const bool interior = prow >= 1 && prow < p.patch_rows - 1 && pcol >= 1 && pcol < p.patch_cols - 1;
                c.terms[pxi] = interior ? value : 0.0f;
            }
            cur_valid_num += (uint32_t)__popcll(wave_ballot(ok));
        }
        cur_valid_num = block_total(b, cur_valid_num, c.wave_cnt);
        if (cur_valid_num == 0) {
            break;
        }
        if (p.consider_luminance) {
            chain_sums(b, c.terms, 1, p.Ppad, c.sums);
            const float cur_average = c.sums[0] / (float)cur_valid_num;
            for (int i = b.tid; i < p.P; i += b.nt) {
                curp[i] /= cur_average;
            }
            blk_sync(b);
        }

        // ComputeHessianAndBias (:197-229)
        uint32_t n_valid = 0;
        for (int base = 0; base < p.P; base += b.nt) {
            const int pxi = base + b.tid;
            bool ok = false;
            if (pxi < p.P) {
                int prow, pcol;
                pixel_rc(p, pxi, prow, pcol);
                const float row_i = (float)(prow - p.half_rows) + ref_v;
                const float col_i = (float)(pcol - p.half_cols) + ref_u;
                const int ei = imul(prow + 1, p.ex_cols) + pcol + 1;
                ok = exv[ei] != 0 && curv[pxi] != 0;
                const float dx = dxs[pxi], dy = dys[pxi];
                lssd_terms(p, c.terms, pxi, ok, lssd_pixel_j0(s, row_i, col_i, dx, dy), dx, dy, curp[pxi] - ex[ei]);
            }
            n_valid += (uint32_t)__popcll(wave_ballot(ok));
        }
        n_valid = block_total(b, n_valid, c.wave_cnt);
        if (n_valid == 0) {
            break;
        }
        chain_then(b, c.terms, 9, p.Ppad, c.sums, false, [&]() { lssd_solve(c.sums, b.lane); });
        float v[3];
        const bool solved = lssd_solve_and_update(c.sums, s, v, status, b.lane);
        blk_sync(b);  // sums[] may be rewritten by the luminance chain of the next iteration
        if (!solved) {
            break;
        }
        if (fast_step_logic(p, vec3_squared_norm(v), last_squared_step, large_step_cnt, status)) {
            break;
        }
    }
}

// TrackOneFeatureFast (lssd_klt_fast.cpp:7-229) for a ONE-WAVE feature without the luminance scaling: the sweep and the chain
// alternate over 64-pixel chunks through a one-slot ring in LDS (9 rows x 64 products) instead of laying all P products of all
// nine chains out first — 2.4 KB of LDS instead of 6.2 KB at 13 x 13, which is what caps the resident features per CU for this
// variant — and the nine sums stay in the chain lanes' registers (lssd_chunked_step).  Same per-pixel expressions, same row-major
// order of every sum as lssd_level_fast: bit-identical.
__device__ __forceinline__ void lssd_level_fast_chunked(const Blk &b, const KltParams &p, const DevImage &ref, const DevImage &cur, float ref_u,
                                                        float ref_v, LssdState &s, uint8_t &status, uint32_t &iters, Carve &c) {
    LssdChunked lv;
    if (!lssd_chunked_entry<false>(b, p, ref, cur, ref_u, ref_v, s, status, c, lv)) {
        return;
    }
    for (uint32_t iter = 0; iter < p.max_iteration; ++iter) {
        ++iters;
        float centre_u, centre_v;
        se2_apply(s, ref_u, ref_v, centre_u, centre_v);
        ensure_cur_window(b, p, cur, centre_u, centre_v, c, lv.cw, lv.cw_staged);
        const bool partly_outside = lssd_partly_outside(p, cur, centre_u, centre_v);
        // lssd_klt_fast.cpp:60-63 / :80-83 only ask whether the two counts are zero (their values feed the luminance scaling,
        // which this variant does not serve): one flag per lane and one ballot per iteration instead of two per chunk
        bool seen_cur = false, seen_valid = false;
        float acc = 0.0f;
        float part[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // throughput mode only (b.tree is a compile-time constant)
        for (int chunk = 0; chunk < lv.n_chunks; ++chunk) {
            const int pxi = chunk * kChunkPixels + b.lane;
            const bool in = pxi < p.P;
            const int pp = in ? pxi : 0;
            const float2 rci = lv.rc[pp];
            const float4 px4 = lv.rec[pp];
            const float row_i = rci.x, col_i = rci.y;
            float row_j, col_j;
            se2_apply(s, col_i, row_i, col_j, row_j);
            float value;
            const bool ok_cur = lssd_sample_cur<true>(cur, lv.cw, row_j, col_j, partly_outside, value) && in;
            const bool ok = __float_as_int(px4.w) != 0 && ok_cur;
            lssd_ring_products(lv.ring, b.lane, ok, s, row_i, col_i, px4, value);
            seen_cur = seen_cur || ok_cur;
            seen_valid = seen_valid || ok;
            blk_sync(b);  // one wave: LDS operations run in program order; this keeps the compiler from reordering across
            if (b.tree) {
                // throughput mode: every lane adds ITS pixel's nine products to nine partial sums (combined by a butterfly below)
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    part[k] += lv.ring[k * kChunkRow + b.lane];
                }
            } else {
                acc = lssd_chain_ring<9>(b, p, lv.ring, chunk, acc);
            }
            blk_sync(b);
        }
        if (b.tree) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    part[k] += __shfl_xor(part[k], off, kWave);
                }
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                acc = (b.lane == k * sum_lanes(p)) ? part[k] : acc;  // the sums where the exact path leaves them: lanes 0..8 (quad chains: 0, 4 .. 32)
            }
        }
        if (wave_ballot(seen_cur) == 0ull || wave_ballot(seen_valid) == 0ull) {
            break;  // lssd_klt_fast.cpp:60-63 / :80-83
        }
        if (!lssd_chunked_step(b, p, acc, s, lv, status)) {
            break;
        }
    }
}

// The same level with consider_patch_luminance (lssd_klt_fast.cpp:27-46, 65-78): the reference patch and its gradients are divided by
// the reference mean once per level (lssd_chunked_entry<true>), the current patch by its mean in every iteration — a SECOND
// exact-order sum per iteration (the interior of the sampled patch, row-major) in front of the nine.  Chunked like the level above:
// pass 1 samples chunk by chunk, keeps each lane's values in REGISTERS (a lane owns the pixels lane, lane + 64, ...: at most
// kLumChunks of them) and chains the mean through ring row 0; pass 2 divides, forms the nine products and chains them.  The quirk
// of the reference is kept: the current mean's numerator covers patch rows / columns 1 .. size - 2 only and its denominator every
// valid pixel.  Same expressions, same order of every sum as lssd_level_fast: bit-identical.
constexpr int kLumChunks = 8;  // 64-pixel chunks a lane can keep values for: patches up to 512 pixels (klt_plan.cpp gates on it)

__device__ __forceinline__ void lssd_level_fast_chunked_lum(const Blk &b, const KltParams &p, const DevImage &ref, const DevImage &cur, float ref_u,
                                                            float ref_v, LssdState &s, uint8_t &status, uint32_t &iters, Carve &c) {
    LssdChunked lv;
    if (!lssd_chunked_entry<true>(b, p, ref, cur, ref_u, ref_v, s, status, c, lv)) {
        return;
    }
    for (uint32_t iter = 0; iter < p.max_iteration; ++iter) {
        ++iters;
        float centre_u, centre_v;
        se2_apply(s, ref_u, ref_v, centre_u, centre_v);
        ensure_cur_window(b, p, cur, centre_u, centre_v, c, lv.cw, lv.cw_staged);
        const bool partly_outside = lssd_partly_outside(p, cur, centre_u, centre_v);
        // ---- pass 1: ExtractPatchInCurrentImage (:145-195) + the mean's numerator (:65-71) ----
        float val[kLumChunks];
        uint32_t ok_mask = 0;  // bit k: this lane's pixel of chunk k was sampled inside the image
        uint32_t cur_valid_num = 0;
        float mean_acc = 0.0f;
#pragma unroll
        for (int chunk = 0; chunk < kLumChunks; ++chunk) {
            val[chunk] = 0.0f;
            if (chunk < lv.n_chunks) {
                const int pxi = chunk * kChunkPixels + b.lane;
                const bool in = pxi < p.P;
                const int pp = in ? pxi : 0;
                const float2 rci = lv.rc[pp];
                float row_j, col_j;
                se2_apply(s, rci.y, rci.x, col_j, row_j);
                float value;
                const bool ok_cur = lssd_sample_cur<true>(cur, lv.cw, row_j, col_j, partly_outside, value) && in;
                int prow, pcol;
                pixel_rc(p, pp, prow, pcol);
                const bool interior = in && prow >= 1 && prow < p.patch_rows - 1 && pcol >= 1 && pcol < p.patch_cols - 1;
                val[chunk] = value;
                ok_mask |= ok_cur ? (1u << chunk) : 0u;
                cur_valid_num += (uint32_t)__popcll(wave_ballot(ok_cur));
                lv.ring[b.lane] = interior ? value : 0.0f;
                blk_sync(b);
                mean_acc = lssd_chain_ring<1>(b, p, lv.ring, chunk, mean_acc);  // quad chain: every quad carries the one sum
                blk_sync(b);
            }
        }
        if (cur_valid_num == 0) {
            break;  // :60-63
        }
        const float cur_average = bcast_lane(mean_acc, 0) / (float)cur_valid_num;
        // ---- pass 2: the scaled patch (:72-78) and ComputeHessianAndBias (:197-229) ----
        bool seen_valid = false;
        float acc = 0.0f;
#pragma unroll
        for (int chunk = 0; chunk < kLumChunks; ++chunk) {
            if (chunk < lv.n_chunks) {
                const int pxi = chunk * kChunkPixels + b.lane;
                const int pp = pxi < p.P ? pxi : 0;
                const float2 rci = lv.rc[pp];
                const float4 px4 = lv.rec[pp];
                const bool ok = __float_as_int(px4.w) != 0 && ((ok_mask >> chunk) & 1u) != 0u;
                lssd_ring_products(lv.ring, b.lane, ok, s, rci.x, rci.y, px4, val[chunk] / cur_average);
                seen_valid = seen_valid || ok;
                blk_sync(b);
                acc = lssd_chain_ring<9>(b, p, lv.ring, chunk, acc);
                blk_sync(b);
            }
        }
        if (wave_ballot(seen_valid) == 0ull) {
            break;  // :80-83
        }
        if (!lssd_chunked_step(b, p, acc, s, lv, status)) {
            break;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Per-feature driver: TrackMultipleLevel / TrackSingleLevel of the three trackers
// (basic_klt.cpp:7-86, affine_klt.cpp:6-91, lssd_klt.cpp:7-94).
// ---------------------------------------------------------------------------------------------
template <int MODEL>
struct ChainCount;
template <>
struct ChainCount<FTK_MODEL_BASIC> {
    static constexpr int value = 5;
};
template <>
struct ChainCount<FTK_MODEL_AFFINE> {
    static constexpr int value = A_COUNT;
};
template <>
struct ChainCount<FTK_MODEL_LSSD> {
    static constexpr int value = 9;
};

constexpr int kMaxWaves = 4;
constexpr int kLongFeatureSlots = 128;  // launch slots (longest first) that keep the top issue priority

// Register cap: the compiler is asked to fit kWavesPerEu waves per SIMD so that enough feature
// workgroups are co-resident per CU (the kernel is issue / latency bound, not register bound).
constexpr int kWavesPerEu = 4;  // <= 128 VGPRs: 8 two-wave (or 4 four-wave) feature workgroups per CU
#define FTK_EU_ATTR __attribute__((amdgpu_waves_per_eu(kWavesPerEu)))

// (The non-fast affine variants used to need a cap of 3 — 168 VGPRs, 24 of them row pointers of the product stores; with the
// grouped product layout, affine_all_terms, they fit 128 like the rest.)
// SOLO: the one-wave-per-feature instantiation (workgroup = one wavefront): compile-time, so that no barrier and no cross-wave
// exchange is left in it.
// H: the half patch size (rows == columns) as a compile-time constant — 6, the reference's default (optical_flow.h:24-25) and
// the patch of BASELINE configurations 3 and 4, is instantiated — or 0 for "as passed".  With it the patch / window geometry
// folds into immediates (klt_fill_geometry, the function the host filled the argument with) instead of occupying SGPRs, most
// of which the register allocator otherwise spills to vector lanes.
// TREE: the throughput mode (ftk_set_reduction_mode; KltParams::tree) as a compile-time property, so that the contract path's
// instantiations contain none of its code: the chain helpers and the chunked LSSD level sum by per-lane partials + a butterfly
// instead of in the reference's order.  The non-fast affine variants ignore it (their 24 sums of 169 terms already run as 24
// parallel chains; a butterfly over so few pixels is not faster) and stay exact.  Run-time geometry only (H == 0).
// LUM: the chunked LSSD-fast level with consider_patch_luminance (its own instantiations, so that the plain chunked level keeps its
// register count: the luminance form holds a lane's sampled values across its two passes).
// SPILL: the large-patch form (KltParams::spill; multi-wave, run-time geometry, exact sums only): carve_spill instead of carve_lds.
template <int MODEL, int METHOD, bool SOLO, int H, bool TREE = false, bool LUM = false, bool SPILL = false>
__global__ void FTK_EU_ATTR __launch_bounds__(kWave *kMaxWaves) klt_track_kernel(const KltParams p_arg) {
    // `p` carries everything but the level tables, which stay in the kernel argument: a local copy whose arrays are indexed
    // with a run-time level would live in scratch memory
    klt_touch_kernarg<sizeof(KltParams)>();  // every line of the argument block requested up front (klt_scalar.h)
    KltParams p = p_arg;
    if constexpr (H > 0) {
        p.half_rows = H;
        p.half_cols = H;
        klt_fill_geometry(p);
        p.a0_floats = p_arg.a0_floats;  // the host overrides it for the chunked LSSD variant (its extended patch lives in the ring's space)
    }
    extern __shared__ float4 lds_raw[];
    Blk b;
    b.solo = SOLO;
    b.tree = TREE;
    b.tid = SOLO ? (int)(threadIdx.x & (kWave - 1)) : (int)threadIdx.x;
    b.nt = SOLO ? kWave : (int)blockDim.x;
    b.lane = b.tid & (kWave - 1);
    b.wave = SOLO ? 0 : b.tid >> 6;
    b.nwaves = SOLO ? 1 : b.nt >> 6;
    // SOLO: p.features_per_group one-wave features share a workgroup without ever meeting (own LDS carve, no barrier)
    // block 0 of a launch that carries the previous call's iteration counts sorts them into a later call's launch order
    // (klt_order.h) beside the feature workgroups; the feature blocks follow it
    uint32_t block = blockIdx.x;
    if (p.sort_iters) {
        if (block == 0) {
            klt_order_block(p.sort_iters, p.sort_order_out, p.n, reinterpret_cast<int *>(lds_raw), p.sort_ref_uv, p_arg.ref[0].cols, p_arg.ref[0].rows, SOLO ? max(p.features_per_group, 1) : 1,
                            p.sched_flags, p.sched_call);
            return;
        }
        block -= 1;
    }
    // launch slot -> feature: in list order, or through the longest-first permutation of an earlier call's iteration counts
    const uint32_t slot_id = SOLO ? block * (uint32_t)p.features_per_group + (threadIdx.x >> 6) : block;
    if (slot_id >= (uint32_t)p.n) {
        return;
    }
    // ... and, for callers whose list changes between frames, a trade of places between an early slot and a late one whose
    // POSITION predicts many iterations (klt_order.h sched_resolve_slot; one wave decides for the workgroup)
    uint32_t list_slot = slot_id;
    bool swapped_in = false;
    if (p.sched_claim != nullptr) {
        if (SOLO) {
            list_slot = sched_resolve_slot(p, slot_id, swapped_in);
        } else {
            uint32_t *const shared = reinterpret_cast<uint32_t *>(lds_raw);
            if (b.wave == 0) {
                const uint32_t r = sched_resolve_slot(p, slot_id, swapped_in);
                if (b.lane == 0) {
                    shared[0] = r;
                    shared[1] = swapped_in ? 1u : 0u;
                }
            }
            __syncthreads();
            list_slot = shared[0];
            swapped_in = shared[1] != 0u;
            __syncthreads();  // the words belong to the carve below
        }
    }
    const uint32_t id = p.order ? (uint32_t)p.order[list_slot] : list_slot;
    // the three per-feature inputs are requested together (one global round trip, not two one after the other)
    const float2 in_uv = reinterpret_cast<const float2 *>(p.cur_uv_in)[id];
    const float2 full_ref = reinterpret_cast<const float2 *>(p.ref_uv)[id];
    uint8_t status = p.status_in[id];
    const float in_u = in_uv.x, in_v = in_uv.y;
    // features beyond kMaxTrackPointsNumber and features that already failed are passed through
    if (id >= p.n_track || status > FTK_TRACKED) {
        if (b.tid == 0) {
            p.cur_uv_out[2 * id] = in_u;
            p.cur_uv_out[2 * id + 1] = in_v;
            p.status_out[id] = status;
            if (p.iters) {
                p.iters[id] = 0;
            }
            if (p.sched_iters) {
                p.sched_iters[id] = 0;
            }
        }
        return;
    }

    constexpr int K = ChainCount<MODEL>::value;
    float *lds_mine = reinterpret_cast<float *>(lds_raw);
    if (SOLO && p.features_per_group > 1) {
        lds_mine += (size_t)(threadIdx.x >> 6) * (p.group_lds_stride >> 2);
    }
    Carve c = SPILL ? carve_spill(lds_mine, p.spill_base + (size_t)block * p.spill_stride_floats, K, p) : carve_lds(lds_mine, K, p);
    if (MODEL == FTK_MODEL_AFFINE && METHOD != FTK_METHOD_FAST) {
        if (p.a0_floats == 0) {
            c.a0 = c.terms;  // the level setup's axis tables share the head of the product groups (a0_floats == 0: klt_plan.cpp)
        }
        // grouped layout (affine_all_terms): the pixels behind the patch up to the end of the last round of groups, all 24 sums
        const int first = p.P, end = affine_group_rounds(p.Ppad) * (4 * kChainRound);
        for (int idx = b.tid; idx < A_COUNT * (end - first); idx += b.nt) {
            const int k = idx / (end - first);
            const int pxi = first + (idx - k * (end - first));
            c.terms[(pxi >> 2) * kAffineGroup + 4 * k + (pxi & 3)] = 0.0f;
        }
    } else if (!(SOLO && p.lssd_chunked)) {
        zero_term_padding(b, c.terms, K, p);
    }

    const float full_ref_u = full_ref.x, full_ref_v = full_ref.y;
    const float scale = p.single_level ? 1.0f : (float)(1 << (p.n_levels - 1));
    float ref_u = p.single_level ? full_ref_u : full_ref_u / scale;
    float ref_v = p.single_level ? full_ref_v : full_ref_v / scale;
    const float scur_u = p.single_level ? in_u : in_u / scale;
    const float scur_v = p.single_level ? in_v : in_v / scale;

    BasicState bs = {scur_u, scur_v};
    AffineState as = {scur_u, scur_v, 1.0f, 0.0f, 0.0f, 1.0f};
    if (p.single_level) {
        as.a00 = p.prior[0];  // affine_klt.cpp:70 — the prediction is only honoured on the single-level path
        as.a01 = p.prior[1];
        as.a10 = p.prior[2];
        as.a11 = p.prior[3];
    }
    LssdState ls;
    ls.r00 = p.prior[0];
    ls.r01 = p.prior[1];
    ls.r10 = p.prior[2];
    ls.r11 = p.prior[3];
    ls.t0 = scur_u - (p.prior[0] * ref_u + p.prior[1] * ref_v);  // lssd_klt.cpp:23
    ls.t1 = scur_v - (p.prior[2] * ref_u + p.prior[3] * ref_v);

    uint32_t iters = 0;
    float out_u = in_u, out_v = in_v;
    const Blk &b0 = b;
    for (int level = p.n_levels - 1; level > -1; --level) {
        const DevImage ref = p_arg.ref[level];
        const DevImage cur = p_arg.cur[level];
        blk_sync(b);  // the previous level's readers of the LDS windows / arrays are done
        const Blk b = opaque_blk(b0);  // per-thread index math stays inside the level (see opaque())
        // the features the launch order put first are the ones expected to run longest — the launch ends when they do — so
        // they keep the top issue priority on their SIMDs at every level
        // (the later-dispatched-half boost of the pipelined kernel was measured here too: Basic direct / fast -2...-4 %, the affine and
        // LSSD variants +1 % — their launches end with their longest feature, not with their youngest; not taken)
        set_level_priority(((p.order && slot_id < (uint32_t)kLongFeatureSlots) || swapped_in) ? 3 : level);
        if (MODEL == FTK_MODEL_BASIC) {
            if (METHOD == FTK_METHOD_FAST) {
                basic_level_fast(b, p, ref, cur, ref_u, ref_v, bs, status, iters, c);
            } else {
                basic_level<METHOD>(b, p, ref, cur, ref_u, ref_v, bs, status, iters, c);
            }
        } else if (MODEL == FTK_MODEL_AFFINE) {
            if (METHOD == FTK_METHOD_FAST) {
                affine_level_fast(b, p, ref, cur, ref_u, ref_v, as, status, iters, c);
            } else {
                affine_level<METHOD>(b, p, ref, cur, ref_u, ref_v, as, status, iters, c);
            }
        } else {
            if (METHOD == FTK_METHOD_FAST) {
                if constexpr (LUM) {
                    lssd_level_fast_chunked_lum(b, p, ref, cur, ref_u, ref_v, ls, status, iters, c);
                } else if (SOLO && p.lssd_chunked) {
                    lssd_level_fast_chunked(b, p, ref, cur, ref_u, ref_v, ls, status, iters, c);
                } else {
                    lssd_level_fast(b, p, ref, cur, ref_u, ref_v, ls, status, iters, c);
                }
            } else {
                lssd_level<METHOD>(b, p, ref, cur, ref_u, ref_v, ls, status, iters, c);
            }
        }

        if (level == 0) {
            if (MODEL == FTK_MODEL_BASIC) {
                out_u = bs.cur_u;
                out_v = bs.cur_v;
            } else if (MODEL == FTK_MODEL_AFFINE) {
                out_u = as.cur_u;
                out_v = as.cur_v;
            } else if (!p.single_level) {
                // lssd_klt.cpp:43 — written back with the UNSCALED ref; the single-level path
                // never writes cur_pixel_uv (lssd_klt.cpp:72-89, sic)
                out_u = (ls.r00 * full_ref_u + ls.r01 * full_ref_v) + ls.t0;
                out_v = (ls.r10 * full_ref_u + ls.r11 * full_ref_v) + ls.t1;
            }
            break;
        }
        ref_u *= 2.0f;
        ref_v *= 2.0f;
        if (MODEL == FTK_MODEL_BASIC) {
            bs.cur_u *= 2.0f;
            bs.cur_v *= 2.0f;
        } else if (MODEL == FTK_MODEL_AFFINE) {
            as.cur_u *= 2.0f;
            as.cur_v *= 2.0f;
        } else {
            ls.t0 *= 2.0f;
            ls.t1 *= 2.0f;
        }
    }

    if (uv_outside(out_u, out_v, p_arg.cur[0])) {
        status = FTK_OUTSIDE;
    }
    if (b.tid == 0) {
        p.cur_uv_out[2 * id] = out_u;
        p.cur_uv_out[2 * id + 1] = out_v;
        p.status_out[id] = status;
        if (p.iters) {
            p.iters[id] = iters;
        }
        tail_report(p, iters, id);  // the longest feature of the call, for the next call's wave policy
        sched_grid_record(p, full_ref_u, full_ref_v, out_u, out_v, iters);  // ... and by position
        if (p.sched_iters) {
            p.sched_iters[id] = iters;  // the next call's launch order (ftk_klt.cpp: longest first)
        }
    }
}

// The generic kernel's instantiation for a plan.
template <int MODEL, int METHOD>
KltKernel pick_variant(const KltPlan &plan, const KltParams &p) {
    const bool solo = p.waves_per_feature == 1;
    if (plan.form == KltForm::GenericSpill) {
        return {klt_track_kernel<MODEL, METHOD, false, 0, false, false, true>, "generic", 0, false, false, false, true};
    }
    if (p.tree) {  // throughput mode (reported, never the contract): its own instantiations, run-time geometry
        return solo ? KltKernel{klt_track_kernel<MODEL, METHOD, true, 0, true>, "generic", 0, true, true, false, false}
                    : KltKernel{klt_track_kernel<MODEL, METHOD, false, 0, true>, "generic", 0, false, true, false, false};
    }
    // (measured per variant, 13 x 13: Basic -6...-14 %, LSSD -16...-21 %, affine fast -16 %, affine inverse / direct -8...-9 % — the
    // latter only once chain_groups' loop is kept rolled: with a compile-time round count the compiler unrolled it fully and the
    // kernel went from 81 to 128 VGPRs and 9...18 % SLOWER)
    bool h6 = p.half_rows == 6 && p.half_cols == 6;
    if (h6) {
        KltParams check = p;
        klt_fill_geometry(check);  // what the specialised kernel recomputes: it must be what the caller passed
        h6 = check.cwin_rows == p.cwin_rows && check.cwin_cols == p.cwin_cols && check.Ppad == p.Ppad && check.rwin_cols == p.rwin_cols;
    }
    if constexpr (MODEL == FTK_MODEL_LSSD && METHOD == FTK_METHOD_FAST) {
        if (solo && p.lssd_chunked && p.consider_luminance) {
            return h6 ? KltKernel{klt_track_kernel<MODEL, METHOD, true, 6, false, true>, "generic", 6, true, false, true, false}
                      : KltKernel{klt_track_kernel<MODEL, METHOD, true, 0, false, true>, "generic", 0, true, false, true, false};
        }
    }
    if (h6) {
        return solo ? KltKernel{klt_track_kernel<MODEL, METHOD, true, 6>, "generic", 6, true, false, false, false}
                    : KltKernel{klt_track_kernel<MODEL, METHOD, false, 6>, "generic", 6, false, false, false, false};
    }
    return solo ? KltKernel{klt_track_kernel<MODEL, METHOD, true, 0>, "generic", 0, true, false, false, false}
                : KltKernel{klt_track_kernel<MODEL, METHOD, false, 0>, "generic", 0, false, false, false, false};
}

int chain_count(int model) {
    switch (model) {
        case FTK_MODEL_BASIC: return ChainCount<FTK_MODEL_BASIC>::value;
        case FTK_MODEL_AFFINE: return ChainCount<FTK_MODEL_AFFINE>::value;
        case FTK_MODEL_LSSD: return ChainCount<FTK_MODEL_LSSD>::value;
        default: return 0;
    }
}

}  // namespace

size_t klt_generic_feature_lds_bytes(int model, const KltParams &p) {
    const int k = chain_count(model);
    return k == 0 ? 0 : (carve_bytes(k, p) + 15) & ~(size_t)15;
}

size_t klt_spill_lds_bytes(int model, const KltParams &p) { return chain_count(model) == 0 ? 0 : (spill_lds_bytes(p) + 15) & ~(size_t)15; }

size_t klt_spill_floats(int model, const KltParams &p) {
    const int k = chain_count(model);
    return k == 0 ? 0 : (spill_floats(k, p) + 3) & ~(size_t)3;
}

namespace {
// Test hook for the lane-parallel 6x6 LDLT: one wave per system.
__global__ void __launch_bounds__(kWave) ldlt6_kernel(const float *a, const float *b, float *x, int n) {
    __shared__ float sa[36], sb[6], sx[6];
    const int sys = blockIdx.x;
    if (sys >= n) {
        return;
    }
    if (threadIdx.x < 36) {
        sa[threadIdx.x] = a[(size_t)sys * 36 + threadIdx.x];
    }
    if (threadIdx.x < 6) {
        sb[threadIdx.x] = b[(size_t)sys * 6 + threadIdx.x];
    }
    __syncthreads();
    const Ldlt6 f = ldlt6_factor(sa, (int)threadIdx.x);
    ldlt6_solve(f, sb, sx, (int)threadIdx.x);
    __syncthreads();
    if (threadIdx.x < 6) {
        x[(size_t)sys * 6 + threadIdx.x] = sx[threadIdx.x];
    }
}
}  // namespace

hipError_t ldlt6_launch(const float *a, const float *b, float *x, int n, hipStream_t stream) {
    if (n <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(ldlt6_kernel, dim3((unsigned)n), dim3(kWave), 0, stream, a, b, x, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------
// Launch order from POSITIONS, made before the launch (two small kernels).  The index-keyed order above needs the same feature
// COUNT three calls in a row; a front end drops and re-detects features every frame, so its calls never get one and run in list
// order ("cold": config 4 199 us against 147).  Every tracker kernel leaves a feature's iteration count in the position table
// (sched_grid_record); here every feature of THIS call looks its reference position up in the table the LAST call wrote, the
// counts are binned, and the features are dealt to launch slots longest first — a counting sort whose order inside a bin is whatever
// the atomics make it (which slot runs a feature changes nothing in its arithmetic).
// ---------------------------------------------------------------------------------------------------------------------------
namespace {
// Adds of many lanes to few addresses are combined per wave first: one atomic per (wave, distinct bin), the lanes of a bin ranked by
// lane number — atomics to ONE address serialise at ~11 ns each chip-wide (25 000 features with equal counts took 300 us lane by lane).
// Returns this lane's rank among the wave's lanes of its bin and, through `group_size` / `leader`, the size of that group and whether
// this lane speaks for it.
__device__ __forceinline__ uint32_t wave_bin_rank(uint32_t bin, bool active, uint32_t &group_size, bool &leader) {
    const int lane = (int)(threadIdx.x & 63);
    uint32_t rank = 0;
    group_size = 0;
    leader = false;
    unsigned long long todo = __ballot(active);
    while (todo != 0ull) {  // wave-uniform: one trip per distinct bin among the active lanes
        const int first = (int)__builtin_ctzll(todo);
        const uint32_t b0 = (uint32_t)__shfl((int)bin, first);
        const unsigned long long same = __ballot(active && bin == b0);
        if (active && bin == b0) {
            rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
            group_size = (uint32_t)__popcll(same);
            leader = lane == first;
        }
        todo &= ~same;
    }
    return rank;
}

__global__ void __launch_bounds__(256) klt_predict_hist_kernel(const float *ref_uv, int n, const uint32_t *table, uint32_t last_call, uint8_t *pred,
                                                               uint32_t *hist) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    uint32_t count = 0;
    if (i < n) {
        const uint32_t word = table[sched_table_slot(ref_uv[2 * i], ref_uv[2 * i + 1])];
        count = (word >> 8) == (last_call & 0xFFFFFFu) ? (word & 0xFFu) : 0u;
        pred[i] = (uint8_t)count;
    }
    uint32_t group_size;
    bool leader;
    (void)wave_bin_rank(count, i < n, group_size, leader);
    if (leader) {
        atomicAdd(&hist[count], group_size);
    }
}

__global__ void __launch_bounds__(256) klt_predict_scatter_kernel(const uint8_t *pred, int n, const uint32_t *hist, uint32_t *cursor, int32_t *order) {
    __shared__ uint32_t counts[256], start[256];
    counts[threadIdx.x] = hist[threadIdx.x];
    __syncthreads();
    {
        // first launch slot of bin b: the features of every LARGER count come first
        uint32_t before = 0u;
        for (int b = 255; b > (int)threadIdx.x; --b) {
            before += counts[b];
        }
        start[threadIdx.x] = before;
    }
    __syncthreads();
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const uint32_t b = i < n ? pred[i] : 0u;
    uint32_t group_size;
    bool leader;
    const uint32_t rank = wave_bin_rank(b, i < n, group_size, leader);
    uint32_t base = 0;
    if (leader) {
        base = atomicAdd(&cursor[b], group_size);
    }
    // the leader's base reaches its group: every lane reads it from the first lane of ITS bin (all 64 lanes take part in the shuffles)
    unsigned long long todo = __ballot(i < n);
    uint32_t my_base = 0;
    while (todo != 0ull) {
        const int first = (int)__builtin_ctzll(todo);
        const uint32_t b0 = (uint32_t)__shfl((int)b, first);
        const uint32_t base0 = (uint32_t)__shfl((int)base, first);
        const unsigned long long same = __ballot(i < n && b == b0);
        if (i < n && b == b0) {
            my_base = base0;
        }
        todo &= ~same;
    }
    if (i < n) {
        const uint32_t slot = start[b] + my_base + rank;
        order[slot < (uint32_t)n ? slot : 0u] = i;  // (slot < n always: the bins hold exactly n features)
    }
}
}  // namespace

hipError_t klt_position_order_launch(const float *ref_uv, int32_t n, const uint32_t *last_table, uint32_t last_call, uint8_t *pred, uint32_t *hist_and_cursor,
                                     int32_t *order, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(hist_and_cursor, 0, sizeof(uint32_t) * kSchedOrderWords, stream);
    if (e != hipSuccess) {
        return e;
    }
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(klt_predict_hist_kernel, dim3(blocks), dim3(256), 0, stream, ref_uv, n, last_table, last_call, pred, hist_and_cursor);
    hipLaunchKernelGGL(klt_predict_scatter_kernel, dim3(blocks), dim3(256), 0, stream, pred, n, hist_and_cursor, hist_and_cursor + 256, order);
    return hipGetLastError();
}

KltKernel klt_pick(const KltPlan &plan, int model, int method, const KltParams &p) {
    if (plan.form == KltForm::Pipelined) {
        return klt_pipelined_pick(p);
    }
    if (plan.form == KltForm::OneWaveFast) {
        return klt_fast_pick(model, p);
    }
    const int m = (method == FTK_METHOD_INVERSE || method == FTK_METHOD_DIRECT) ? method : FTK_METHOD_FAST;
#define FTK_DISPATCH(MODEL)                                                             \
    switch (m) {                                                                        \
        case FTK_METHOD_INVERSE: return pick_variant<MODEL, FTK_METHOD_INVERSE>(plan, p); \
        case FTK_METHOD_DIRECT: return pick_variant<MODEL, FTK_METHOD_DIRECT>(plan, p);   \
        default: return pick_variant<MODEL, FTK_METHOD_FAST>(plan, p);                    \
    }
    switch (model) {
        case FTK_MODEL_BASIC: FTK_DISPATCH(FTK_MODEL_BASIC)
        case FTK_MODEL_AFFINE: FTK_DISPATCH(FTK_MODEL_AFFINE)
        case FTK_MODEL_LSSD: FTK_DISPATCH(FTK_MODEL_LSSD)
        default: return KltKernel{};
    }
#undef FTK_DISPATCH
}

// The one launch path of the trackers: every form's kernel leaves through here.
hipError_t klt_launch(const KltPlan &plan, int model, int method, const KltParams &p, hipStream_t stream) {
    const KltKernel kernel = klt_pick(plan, model, method, p);
    // an inconsistent plan is refused, not repaired (klt_plan sets these fields)
    if (!kernel.entry || p.waves_per_feature < 1 || p.waves_per_feature > kMaxWaves || p.features_per_group < 1 ||
        (p.waves_per_feature > 1 && p.features_per_group != 1) || plan.block != (unsigned)(kWave * p.waves_per_feature * p.features_per_group) ||
        plan.grid != (unsigned)((p.n + p.features_per_group - 1) / p.features_per_group) ||
        (plan.form == KltForm::GenericSpill && (p.waves_per_feature < 2 || !p.spill_base))) {
        return hipErrorInvalidValue;
    }
    const unsigned sort_block = p.sort_iters ? 1u : 0u;  // one more workgroup: the sort of a later call's launch order
    const size_t lds = sort_block && plan.lds_bytes < (size_t)kOrderLdsBytes ? (size_t)kOrderLdsBytes : plan.lds_bytes;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel.entry), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            return e;
        }
    }
    hipLaunchKernelGGL(kernel.entry, dim3(plan.grid + sort_block), dim3(plan.block), lds, stream, p);
    return hipGetLastError();
}

// First-use cost out of the callers' timed regions (ftk_warmup): launching this empty kernel makes the runtime load this
// translation unit's code object onto the device, which otherwise happens inside the first real call.
__global__ void klt_warm_kernel() {}
hipError_t klt_warm(hipStream_t stream) {
    hipLaunchKernelGGL(klt_warm_kernel, dim3(1), dim3(64), 0, stream);
    return hipGetLastError();
}

}  // namespace ftk
