// klt_window.h — the pixel-pair image window in LDS (Win), the reference's bilinear samplers on it (fetch4 .. sample, the
// branch-free tap and the per-level axis tables), patch pixel geometry and the window-covers-the-footprint test.
// Used by klt_kernels.hip and klt_fast_kernels.hip; klt_basic_kernels.hip (byte windows, its own taps) takes the axes, the
// patch geometry and the cover test.  How a window is filled: klt_stage.h.
#pragma once

#include "klt_scalar.h"

#include <math.h>

namespace ftk {
namespace {

// An image window resident in LDS.  Element (r, c) packs the pixel pair
// (img[clamp(r_lo + r)][clamp(c_lo + c)], img[clamp(r_lo + r)][clamp(c_lo + c + 1)]) into 16 bits,
// clamp = clamp-to-edge, so the 2x2 neighbourhood of any in-image pixel is two ds_read_u16.
struct Win {
    const uint16_t *data;
    int r_lo, c_lo;
    int rows, cols;  // wave-uniform
    // floor(v) in [cover[0], cover[1]] and floor(u) in [cover[2], cover[3]]: the footprint of a patch centred at (u, v) lies inside
    // this window (win_set_cover; an empty interval when the window's origin is too large for the test to be exact in fp32)
    float cover[4];
};

// The 2x2 neighbourhood of the in-image pixel (r0, c0), +1 neighbours clamped to the image:
// from the LDS window when it covers the pixel, from global memory otherwise.
__device__ __forceinline__ void fetch4(const DevImage &im, const Win &w, int r0, int c0, float &p00, float &p01, float &p10, float &p11) {
    const int lr = (int)((unsigned)r0 - (unsigned)w.r_lo);
    const int lc = (int)((unsigned)c0 - (unsigned)w.c_lo);
    if ((unsigned)lr < (unsigned)(w.rows - 1) && (unsigned)lc < (unsigned)w.cols) {
        const int top = imul(lr, w.cols) + lc;  // the row below is one pitch further (not a second multiply of lr + 1)
        const unsigned a = w.data[top];
        const unsigned bb = w.data[top + w.cols];
        p00 = (float)(a & 0xFFu);
        p01 = (float)(a >> 8);
        p10 = (float)(bb & 0xFFu);
        p11 = (float)(bb >> 8);
    } else {
        const int r1 = (r0 + 1 < im.rows) ? r0 + 1 : r0;
        const int c1 = (c0 + 1 < im.cols) ? c0 + 1 : c0;
        p00 = px(im, r0, c0);
        p01 = px(im, r0, c1);
        p10 = px(im, r1, c0);
        p11 = px(im, r1, c1);
    }
}

// GrayImage::GetPixelValueNoCheck(float, float): bilinear, ((tl + tr) + bl) + br, any coordinates
__device__ __forceinline__ float bilinear(const DevImage &im, const Win &w, float row, float col) {
    int r0 = f2i(row);
    int c0 = f2i(col);
    const float sub_row = row - floor_from_trunc(row, r0);
    const float sub_col = col - floor_from_trunc(col, c0);
    r0 = clampi(r0, 0, im.rows - 1);
    c0 = clampi(c0, 0, im.cols - 1);
    const float inv_sub_row = 1.0f - sub_row;
    const float inv_sub_col = 1.0f - sub_col;
    const float w_tl = inv_sub_row * inv_sub_col;
    const float w_tr = inv_sub_row * sub_col;
    const float w_bl = sub_row * inv_sub_col;
    const float w_br = sub_row * sub_col;
    float p00, p01, p10, p11;
    fetch4(im, w, r0, c0, p00, p01, p10, p11);
    return w_tl * p00 + w_tr * p01 + w_bl * p10 + w_br * p11;
}

// bilinear() for coordinates the caller knows to be inside the image with room for the +1 neighbours (0 <= row <= rows - 2,
// 0 <= col <= cols - 2, finite): truncation is floor there and no index needs clamping, so the same values come out of fewer
// instructions.
__device__ __forceinline__ float bilinear_inside(const DevImage &im, const Win &w, float row, float col) {
    const int r0 = (int)row;
    const int c0 = (int)col;
    // x - (float)(int)x for 0 <= x < 2^31 is x - floor(x), exact in fp32, and that is what v_fract_f32 returns (its clamp below
    // 1.0 only matters for tiny negative x): one instruction instead of a conversion and a subtraction, same bits
    const float sub_row = __builtin_amdgcn_fractf(row);
    const float sub_col = __builtin_amdgcn_fractf(col);
    const float inv_sub_row = 1.0f - sub_row;
    const float inv_sub_col = 1.0f - sub_col;
    const float w_tl = inv_sub_row * inv_sub_col;
    const float w_tr = inv_sub_row * sub_col;
    const float w_bl = sub_row * inv_sub_col;
    const float w_br = sub_row * sub_col;
    float p00, p01, p10, p11;
    fetch4(im, w, r0, c0, p00, p01, p10, p11);
    return w_tl * p00 + w_tr * p01 + w_bl * p10 + w_br * p11;
}

// GrayImage::GetPixelValue(row, col, *value): closed-rectangle validity, NaN invalid.  Inside the
// rectangle truncation equals floor, so the fractions need no floor fix-up.
__device__ __forceinline__ bool sample(const DevImage &im, const Win &w, float row, float col, float &value) {
    if (!(row >= 0.0f && col >= 0.0f && row <= (float)(im.rows - 1) && col <= (float)(im.cols - 1))) {
        return false;
    }
    const int r0 = (int)row;
    const int c0 = (int)col;
    const float sub_row = __builtin_amdgcn_fractf(row);  // == row - (float)r0 for row >= 0, see bilinear_inside
    const float sub_col = __builtin_amdgcn_fractf(col);
    const float inv_sub_row = 1.0f - sub_row;
    const float inv_sub_col = 1.0f - sub_col;
    const float w_tl = inv_sub_row * inv_sub_col;
    const float w_tr = inv_sub_row * sub_col;
    const float w_bl = sub_row * inv_sub_col;
    const float w_br = sub_row * sub_col;
    float p00, p01, p10, p11;
    fetch4(im, w, r0, c0, p00, p01, p10, p11);
    value = w_tl * p00 + w_tr * p01 + w_bl * p10 + w_br * p11;
    return true;
}

// --- straight-line sampling for the hot loops ---------------------------------------------------
// One image axis of a bilinear tap: validity on the closed interval [0, limit], base index, fraction
// and its complement — the same quantities sample() derives, computed without branches.
struct Axis {
    int i0;
    float sub, inv;
    bool valid;
};

__device__ __forceinline__ Axis make_axis(float x, int limit) {
    Axis a;
    a.valid = (x >= 0.0f && x <= (float)limit);
    a.i0 = (int)x;
    a.sub = x - (float)a.i0;
    a.inv = 1.0f - a.sub;
    return a;
}

// Bilinear value of (row axis, col axis) read from the LDS window with NO branch: the LDS index is
// clamped into the window so the read is always safe, and `hit` is cleared when the tap was not
// really covered (the caller then redoes the pixel through sample(), which can reach global memory).
// Same weight products and summation order as sample().
__device__ __forceinline__ float tap(const Win &w, const Axis &ar, const Axis &ac, bool &hit) {
    const int lr = (int)((unsigned)ar.i0 - (unsigned)w.r_lo);
    const int lc = (int)((unsigned)ac.i0 - (unsigned)w.c_lo);
    const bool in = (unsigned)lr < (unsigned)(w.rows - 1) && (unsigned)lc < (unsigned)w.cols;
    hit = hit && in;
    const int idx = in ? imul(lr, w.cols) + lc : 0;
    const unsigned a = w.data[idx];
    const unsigned bb = w.data[idx + w.cols];
    const float w_tl = ar.inv * ac.inv;
    const float w_tr = ar.inv * ac.sub;
    const float w_bl = ar.sub * ac.inv;
    const float w_br = ar.sub * ac.sub;
    return w_tl * (float)(a & 0xFFu) + w_tr * (float)(a >> 8) + w_bl * (float)(bb & 0xFFu) + w_br * (float)(bb >> 8);
}

__device__ __forceinline__ bool uv_outside(float u, float v, const DevImage &im) {
    return u < 0.0f || u > (float)(im.cols - 1) || v < 0.0f || v > (float)(im.rows - 1);
}

// Axis tables: the five reference taps of the inverse methods use, per patch pixel, the row axes of
// (row, row-1, row+1) and the column axes of (col, col-1, col+1).  Those depend on the patch row
// (resp. column) only, so they are computed once per level into LDS — 3*(rows+cols) entries instead
// of 6 axes per pixel — with exactly the expressions of the per-pixel form.  Entry layout (float4):
// x = window-relative base index (int bits, 0 when not covered), y = fraction, z = 1 - fraction,
// w = flags (int bits: 1 = inside the image, 2 = covered by the staged window).
__device__ __forceinline__ void build_axis_tables(const Blk &b, const KltParams &p, const DevImage &im, const Win &w, float u, float v,
                                                  int variants, float4 *tab) {
    const int nr = variants * p.patch_rows, total = nr + variants * p.patch_cols;
    for (int t = b.tid; t < total; t += b.nt) {
        const bool is_row = t < nr;
        const int k = is_row ? t : t - nr;
        const int len = is_row ? p.patch_rows : p.patch_cols;
        const int var = (k >= 2 * len) ? 2 : (k >= len ? 1 : 0);
        const int d = k - var * len;
        float x = (float)(d - (is_row ? p.half_rows : p.half_cols)) + (is_row ? v : u);
        if (var == 1) {
            x = x - 1.0f;
        } else if (var == 2) {
            x = x + 1.0f;
        }
        const Axis a = make_axis(x, (is_row ? im.rows : im.cols) - 1);
        const int rel = (int)((unsigned)a.i0 - (unsigned)(is_row ? w.r_lo : w.c_lo));
        const bool hit = is_row ? (unsigned)rel < (unsigned)(w.rows - 1) : (unsigned)rel < (unsigned)w.cols;
        tab[t] = make_float4(__int_as_float(hit ? rel : 0), a.sub, a.inv, __int_as_float((a.valid ? 1 : 0) | (hit ? 2 : 0)));
    }
}

// tap() on two table entries.
__device__ __forceinline__ float tap_table(const Win &w, const float4 &ar, const float4 &ac) {
    const int idx = imul(__float_as_int(ar.x), w.cols) + __float_as_int(ac.x);
    const unsigned a = w.data[idx];
    const unsigned bb = w.data[idx + w.cols];
    const float w_tl = ar.z * ac.z;
    const float w_tr = ar.z * ac.y;
    const float w_bl = ar.y * ac.z;
    const float w_br = ar.y * ac.y;
    return w_tl * (float)(a & 0xFFu) + w_tr * (float)(a >> 8) + w_bl * (float)(bb & 0xFFu) + w_br * (float)(bb >> 8);
}

// Row and column of patch pixel pxi (row-major), by the plan's magic multipliers instead of a division.
__device__ __forceinline__ void pixel_rc(const KltParams &p, int pxi, int &prow, int &pcol) {
    if (p.magic_pc20 != 0) {  // wave-uniform; v_mul_u32_u24 is full rate, v_mul_hi_u32 a quarter of it
        prow = (int)(__umul24((unsigned)pxi, p.magic_pc20) >> 20);
    } else {
        prow = (p.patch_cols == 1) ? pxi : (int)__umulhi((unsigned)pxi, p.magic_pc);
    }
    pcol = pxi - imul(prow, p.patch_cols);
}

// ---------------------------------------------------------------------------------------------
// Window management
// ---------------------------------------------------------------------------------------------

// Top-left corner of the (2h+4)^2 footprint of a patch centred at (u, v): bilinear bases of the
// patch pixels and of their +-1 neighbours lie in [floor - h - 1, floor + h + 1], plus one for the
// +1 bilinear neighbour.
// (u, v) are the feature's coordinates: the same in every lane of the wave (a wave never serves two features), so the corner is
// handed on as a SCALAR — everything integer that follows from it (window tests, clamps, restaging decisions, address bases)
// then runs on the scalar unit instead of taking vector issue slots.
__device__ __forceinline__ void footprint_origin(const KltParams &p, float u, float v, int &r_lo, int &c_lo) {
    r_lo = __builtin_amdgcn_readfirstlane(wadd(f2i(floorf(v)), -(p.half_rows + 1)));
    c_lo = __builtin_amdgcn_readfirstlane(wadd(f2i(floorf(u)), -(p.half_cols + 1)));
}

// The per-iteration form of "does the current window still cover the patch footprint" as four float compares: with
// need = floor(x) - (half + 1) the integer test need >= lo && need + 2 half + 4 <= lo + extent (+ 1 for columns, whose last pair
// reaches one pixel further) is floor(x) in [lo + half + 1, lo + extent - half - 3 (+ 1)] — exact in fp32 while the bounds are small
// integers; for a window whose origin is not (a feature far outside the image) the interval is empty and the integer test decides.
template <class W>  // Win, or the pipelined kernel's byte window: the same origin and extents
__device__ __forceinline__ void win_set_cover(const KltParams &p, W &w) {
    const bool small = (unsigned)(w.r_lo + (1 << 22)) < (1u << 23) && (unsigned)(w.c_lo + (1 << 22)) < (1u << 23);
    w.cover[0] = small ? (float)(w.r_lo + p.half_rows + 1) : 1.0f;
    w.cover[1] = small ? (float)(w.r_lo + w.rows - p.half_rows - 3) : 0.0f;
    w.cover[2] = small ? (float)(w.c_lo + p.half_cols + 1) : 1.0f;
    w.cover[3] = small ? (float)(w.c_lo + w.cols - p.half_cols - 2) : 0.0f;
}

template <class W>
__device__ __forceinline__ bool win_covers(const W &w, float u, float v) {
    const float fu = floorf(u), fv = floorf(v);
    return fv >= w.cover[0] && fv <= w.cover[1] && fu >= w.cover[2] && fu <= w.cover[3];  // NaN and huge coordinates fail
}

}  // namespace
}  // namespace ftk
