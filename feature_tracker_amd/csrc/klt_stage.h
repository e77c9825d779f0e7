// klt_stage.h — filling an LDS image window from a pyramid level, in two flavours: pixel pairs (klt_window.h Win: klt_kernels.hip,
// klt_fast_kernels.hip) and bytes (klt_basic_kernels.hip).  Each has a path of 8-byte units for windows inside the image, its
// prefetch form (raw loads issued early, stored late) and a clamped per-element path for windows that leave the image.
#pragma once

#include "klt_scalar.h"

namespace ftk {
namespace {

// ---------------------------------------------------------------------------------------------
// What the two flavours share
// ---------------------------------------------------------------------------------------------

// The per-element paths (stage_elements, stage_bytes_elements) load up to kStageBatch elements per thread with every global load
// in flight before the first LDS store (the loop body is branch-free: out-of-range slots read element 0 and are not stored).
// They are the same loop around two element functions and stay written out twice: through one template on the element
// function the compiler schedules both differently.
constexpr int kStageBatch = 4;

// N units of 8 consecutive image bytes per thread, as two dwords each (image columns are not aligned): loaded early, stored late.
template <int N>
struct RawOctets {
    uint32_t x[N], y[N];
};

// ---------------------------------------------------------------------------------------------
// Pixel-pair windows
// ---------------------------------------------------------------------------------------------

// One pixel-pair element of a window: (img[clamp(r)][clamp(c)], img[clamp(r)][clamp(c + 1)]).
__device__ __forceinline__ uint16_t window_element(const DevImage &im, int r_lo, int c_lo, int idx, int wcols, uint32_t magic_cols) {
    const int r = (int)__umulhi((unsigned)idx, magic_cols);
    const int c = idx - imul(r, wcols);
    const int ir = clampi(wadd(r_lo, r), 0, im.rows - 1);
    const int ic = wadd(c_lo, c);
    const int ic0 = clampi(ic, 0, im.cols - 1);
    const int ic1 = clampi(wadd(ic, 1), 0, im.cols - 1);
    const unsigned row_off = __umul24((unsigned)ir, (unsigned)im.cols);  // 32-bit offsets, as in px()
    return (uint16_t)((unsigned)im.data[row_off + (unsigned)ic0] | ((unsigned)im.data[row_off + (unsigned)ic1] << 8));
}

__device__ __forceinline__ void stage_elements(const Blk &b, const DevImage &im, uint16_t *dst, int r_lo, int c_lo, int wcols, uint32_t magic_cols,
                                               int total) {
    for (int base = 0; base < total; base += b.nt * kStageBatch) {
        uint16_t v[kStageBatch];
#pragma unroll
        for (int k = 0; k < kStageBatch; ++k) {
            const int idx = base + k * b.nt + b.tid;
            v[k] = window_element(im, r_lo, c_lo, idx < total ? idx : 0, wcols, magic_cols);
        }
#pragma unroll
        for (int k = 0; k < kStageBatch; ++k) {
            const int idx = base + k * b.nt + b.tid;
            if (idx < total) {
                dst[idx] = v[k];
            }
        }
    }
}

// Fast staging for windows that lie completely inside the image: thread (row, quad) fetches 8
// consecutive bytes with one unaligned global_load_dwordx2, forms the four pixel pairs
// (b0,b1) (b1,b2) (b2,b3) (b3,b4) with v_alignbyte / v_alignbit and stores them with one
// ds_write_b64 (wcols is a multiple of 4).  ~1/4 of the instructions of the per-element path.
__device__ __forceinline__ bool window_inside(const DevImage &im, int r_lo, int c_lo, int wrows, int wcols) {
    return r_lo >= 0 && c_lo >= 0 && (long long)r_lo + wrows <= im.rows && (long long)c_lo + wcols + 4 <= im.cols;
}

// Quad idx of a window of `quads` quads per row: its row and its place in the row (magic_quads: the plan's multiplier for / quads).
__device__ __forceinline__ void quad_rc(int idx, int quads, uint32_t magic_quads, int &r, int &q) {
    r = (quads == 1) ? idx : (int)__umulhi((unsigned)idx, magic_quads);
    q = idx - imul(r, quads);
}

// 8 image bytes b0 .. b7 (x = b0..b3, y = b4..b7) -> the four pixel pairs of a quad.
__device__ __forceinline__ uint2 quad_pairs(uint32_t x, uint32_t y) {
    const uint32_t p0 = x & 0xFFFFu;
    const uint32_t p1 = (x >> 8) & 0xFFFFu;
    const uint32_t p2 = x >> 16;
    const uint32_t p3 = __builtin_amdgcn_alignbyte(y, x, 3) & 0xFFFFu;
    return make_uint2(p0 | (p1 << 16), p2 | (p3 << 16));
}

// One quad of a window that lies inside the image, and where it goes in the window (lds_off, in elements).
__device__ __forceinline__ uint2 load_quad_pairs(const DevImage &im, int r_lo, int c_lo, int idx, int quads, uint32_t magic_quads, int &lds_off,
                                                 int wcols) {
    int r, q;
    quad_rc(idx, quads, magic_quads, r, q);
    const uint8_t *src = im.data + (__umul24((unsigned)(r_lo + r), (unsigned)im.cols) + (unsigned)(c_lo + 4 * q));
    uint32_t x, y;
    __builtin_memcpy(&x, src, 4);
    __builtin_memcpy(&y, src + 4, 4);
    // quad_pairs(x, y), written out: the window offset has to be formed between its two halves for the generic kernels' two-window
    // staging (klt_kernels.hip stage_both_inside) to keep its instruction order
    const uint32_t p0 = x & 0xFFFFu;
    const uint32_t p1 = (x >> 8) & 0xFFFFu;
    const uint32_t p2 = x >> 16;
    const uint32_t p3 = __builtin_amdgcn_alignbyte(y, x, 3) & 0xFFFFu;
    lds_off = imul(r, wcols) + 4 * q;
    return make_uint2(p0 | (p1 << 16), p2 | (p3 << 16));
}

__device__ __forceinline__ void stage_rows_inside(const Blk &b, const DevImage &im, uint16_t *dst, int r_lo, int c_lo, int wrows, int wcols,
                                                  uint32_t magic_quads) {
    const int quads = wcols >> 2;
    const int total = wrows * quads;
    for (int idx = b.tid; idx < total; idx += b.nt) {
        int r, q;
        quad_rc(idx, quads, magic_quads, r, q);
        const uint8_t *src = im.data + (__umul24((unsigned)(r_lo + r), (unsigned)im.cols) + (unsigned)(c_lo + 4 * q));
        uint32_t x, y;
        __builtin_memcpy(&x, src, 4);
        __builtin_memcpy(&y, src + 4, 4);
        *reinterpret_cast<uint2 *>(dst + imul(r, wcols) + 4 * q) = quad_pairs(x, y);
    }
}

__device__ __forceinline__ void stage_any(const Blk &b, const DevImage &im, uint16_t *dst, int r_lo, int c_lo, int wrows, int wcols,
                                          uint32_t magic_cols, uint32_t magic_quads) {
    if (window_inside(im, r_lo, c_lo, wrows, wcols)) {
        stage_rows_inside(b, im, dst, r_lo, c_lo, wrows, wcols, magic_quads);
    } else {
        stage_elements(b, im, dst, r_lo, c_lo, wcols, magic_cols, wrows * wcols);
    }
}

// Window prefetch: raw 8-byte loads issued early, turned into pixel pairs and stored late.
template <int N>
__device__ __forceinline__ void issue_quads(RawOctets<N> &q, const Blk &b, const DevImage &im, int r_lo, int c_lo, int wrows, int wcols,
                                            uint32_t magic_quads) {
    const int quads = wcols >> 2;
    const int total = wrows * quads;
    const int tid = opaque(b.tid);
    const uint8_t *base = im.data + (long long)r_lo * im.cols + c_lo;  // wave-uniform: scalar base + 32-bit lane offset
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int idx = tid + k * b.nt;
        idx = idx < total ? idx : 0;
        int r, qq;
        quad_rc(idx, quads, magic_quads, r, qq);
        const uint8_t *src = base + (size_t)(unsigned)(r * im.cols + 4 * qq);
        __builtin_memcpy(&q.x[k], src, 4);
        __builtin_memcpy(&q.y[k], src + 4, 4);
    }
}

template <int N>
__device__ __forceinline__ void store_quads(const RawOctets<N> &q, const Blk &b, uint16_t *dst, int wrows, int wcols, uint32_t magic_quads) {
    const int quads = wcols >> 2;
    const int total = wrows * quads;
    const int tid = opaque(b.tid);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int idx = tid + k * b.nt;
        if (idx < total) {
            int r, qq;
            quad_rc(idx, quads, magic_quads, r, qq);
            *reinterpret_cast<uint2 *>(dst + imul(r, wcols) + 4 * qq) = quad_pairs(q.x[k], q.y[k]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Byte windows (the pipelined Basic kernel): byte (r, c) of a window is img[clamp(r_lo + r)][clamp(c_lo + c)], rows `pitch` bytes
// apart, pitch a power of two (ftk_device.h klt_byte_pitch).  A row is pitch / 8 units of 8 consecutive image bytes; unit idx sits
// at row idx >> log2(units per row), position idx & (units per row - 1), and at LDS byte 8 * idx: no pair building, no division.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int byte_units_shift(int pitch) { return 28 - __builtin_clz((unsigned)pitch); }  // log2(pitch / 8)

// Image byte offset of unit idx relative to the window's origin: klt_byte_unit_offset (ftk_device.h) on the 24-bit multiplier (rows and
// columns of a level are < 2^24 and the product < 2^32, as in px(): the same value).
__device__ __forceinline__ unsigned byte_unit_offset(int idx, int shift, const DevImage &im) {
    const unsigned r = (unsigned)idx >> shift, u = (unsigned)idx & ((1u << shift) - 1u);
    return __umul24(r, (unsigned)im.cols) + 8u * u;
}

// For windows that pass klt_byte_window_inside: the raw 8-byte loads, issued early ...
template <int N>
__device__ __forceinline__ void issue_octets(RawOctets<N> &q, const Blk &b, const DevImage &im, int r_lo, int c_lo, int wrows, int pitch) {
    const int shift = byte_units_shift(pitch);
    const int total = wrows << shift;
    const int tid = opaque(b.tid);
    const uint8_t *base = im.data + (long long)r_lo * im.cols + c_lo;  // wave-uniform: scalar base + 32-bit lane offset
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int idx = tid + k * b.nt;
        idx = idx < total ? idx : 0;
        const uint8_t *src = base + (size_t)byte_unit_offset(idx, shift, im);
        __builtin_memcpy(&q.x[k], src, 4);  // image columns are not aligned: two dword loads, as the quads
        __builtin_memcpy(&q.y[k], src + 4, 4);
    }
}

// ... and stored late, as they came: one ds_write_b64 per unit.
template <int N>
__device__ __forceinline__ void store_octets(const RawOctets<N> &q, const Blk &b, uint8_t *dst, int wrows, int pitch) {
    const int total = wrows << byte_units_shift(pitch);
    const int tid = opaque(b.tid);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int idx = tid + k * b.nt;
        if (idx < total) {
            *reinterpret_cast<uint2 *>(dst + 8 * idx) = make_uint2(q.x[k], q.y[k]);
        }
    }
}

// Both at once (the coarsest level's reference window, a restaged current window, windows with more units than a thread prefetches).
__device__ __forceinline__ void stage_bytes_inside(const Blk &b, const DevImage &im, uint8_t *dst, int r_lo, int c_lo, int wrows, int pitch) {
    const int shift = byte_units_shift(pitch);
    const int total = wrows << shift;
    const uint8_t *base = im.data + (long long)r_lo * im.cols + c_lo;
    for (int idx = b.tid; idx < total; idx += b.nt) {
        const uint8_t *src = base + (size_t)byte_unit_offset(idx, shift, im);
        uint32_t x, y;
        __builtin_memcpy(&x, src, 4);
        __builtin_memcpy(&y, src + 4, 4);
        *reinterpret_cast<uint2 *>(dst + 8 * idx) = make_uint2(x, y);
    }
}

// Windows that leave the image: four clamped pixels per 32-bit word (what stage_elements puts into the low bytes of its pairs; the
// high byte of pair c is byte c + 1 here, clamped the same way), kStageBatch words per thread in flight.
__device__ __forceinline__ uint32_t byte_window_word(const DevImage &im, int r_lo, int c_lo, int word, int pitch_shift) {
    const int r = word >> (pitch_shift - 2), c = (word & ((1 << (pitch_shift - 2)) - 1)) << 2;
    const int ir = clampi(wadd(r_lo, r), 0, im.rows - 1);
    const unsigned row_off = __umul24((unsigned)ir, (unsigned)im.cols);  // 32-bit offsets, as in px()
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ic = clampi(wadd(c_lo, c + k), 0, im.cols - 1);
        w |= (uint32_t)im.data[row_off + (unsigned)ic] << (8 * k);
    }
    return w;
}

__device__ __forceinline__ void stage_bytes_elements(const Blk &b, const DevImage &im, uint8_t *dst, int r_lo, int c_lo, int wrows, int pitch) {
    const int pitch_shift = byte_units_shift(pitch) + 3;
    const int total = wrows << (pitch_shift - 2);
    uint32_t *const words = reinterpret_cast<uint32_t *>(dst);
    for (int base = 0; base < total; base += b.nt * kStageBatch) {
        uint32_t v[kStageBatch];
#pragma unroll
        for (int k = 0; k < kStageBatch; ++k) {
            const int idx = base + k * b.nt + b.tid;
            v[k] = byte_window_word(im, r_lo, c_lo, idx < total ? idx : 0, pitch_shift);
        }
#pragma unroll
        for (int k = 0; k < kStageBatch; ++k) {
            const int idx = base + k * b.nt + b.tid;
            if (idx < total) {
                words[idx] = v[k];
            }
        }
    }
}

__device__ __forceinline__ void stage_bytes_any(const Blk &b, const DevImage &im, uint8_t *dst, int r_lo, int c_lo, int wrows, int pitch) {
    if (klt_byte_window_inside(im.rows, im.cols, r_lo, c_lo, wrows, pitch)) {
        stage_bytes_inside(b, im, dst, r_lo, c_lo, wrows, pitch);
    } else {
        stage_bytes_elements(b, im, dst, r_lo, c_lo, wrows, pitch);
    }
}

}  // namespace
}  // namespace ftk
