// pyramid_kernels.hip — image-side helpers for gfx950 (MI355X).
//
//  * pyramid_downsample: ImagePyramid::CreateImagePyramid's level step (call sites
//    test/test_optical_flow.cpp:70-71): dst = truncating 2x2 box mean of src, (rows/2, cols/2).
//    A pure streaming kernel (1.25 B moved per source byte): every thread produces 4 adjacent
//    output pixels from two 8-byte row segments, so a wave reads 2 x 512 contiguous bytes.
//  * extract_patch: OpticalFlow::ExtractExtendPatchInReferenceImage (optical_flow.cpp:49-102),
//    exposed because the reference makes it a public method; one wave per call.
#include "ftk_device.h"

#include <limits.h>
#include <math.h>

namespace ftk {
namespace {

constexpr int kBlock = 256;

__global__ void __launch_bounds__(kBlock) downsample_kernel(const uint8_t *__restrict__ src, int src_cols, uint8_t *__restrict__ dst, int dst_rows,
                                                            int dst_cols) {
    // one thread -> up to 4 consecutive output pixels of one output row
    const int groups_per_row = (dst_cols + 3) >> 2;
    const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long total = (long long)groups_per_row * dst_rows;
    if (gid >= total) {
        return;
    }
    const int r = (int)(gid / groups_per_row);
    const int c0 = (int)(gid - (long long)r * groups_per_row) << 2;
    const uint8_t *top = src + (long long)(2 * r) * src_cols + 2 * c0;
    const uint8_t *bottom = top + src_cols;
    uint8_t *out = dst + (long long)r * dst_cols + c0;
    const int n = min(4, dst_cols - c0);
    const bool aligned8 = ((reinterpret_cast<uintptr_t>(top) | reinterpret_cast<uintptr_t>(bottom)) & 7) == 0;
    if (n == 4 && aligned8) {
        const uint2 t = *reinterpret_cast<const uint2 *>(top);
        const uint2 b = *reinterpret_cast<const uint2 *>(bottom);
        const unsigned tw[2] = {t.x, t.y}, bw[2] = {b.x, b.y};
        unsigned packed = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned tv = tw[k >> 1] >> ((k & 1) * 16);
            const unsigned bv = bw[k >> 1] >> ((k & 1) * 16);
            const unsigned sum = (tv & 0xFF) + ((tv >> 8) & 0xFF) + (bv & 0xFF) + ((bv >> 8) & 0xFF);
            packed |= (sum >> 2) << (8 * k);
        }
        if ((reinterpret_cast<uintptr_t>(out) & 3) == 0) {
            *reinterpret_cast<unsigned *>(out) = packed;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                out[k] = (uint8_t)(packed >> (8 * k));
            }
        }
    } else {
        for (int k = 0; k < n; ++k) {
            const unsigned sum = (unsigned)top[2 * k] + top[2 * k + 1] + bottom[2 * k] + bottom[2 * k + 1];
            out[k] = (uint8_t)(sum >> 2);
        }
    }
}

// Every level of a pyramid in ONE launch.  CreateImagePyramid sits inside the reference's timed region, right in front of
// TrackFeatures (test/test_optical_flow.cpp:69-73), and a launch per level costs more in launch gaps than the kernels take at
// camera resolutions (640 x 480: three ~3 us launches for 0.1 MB of work).  A workgroup owns one 64 x 64 tile of level 0; since 64
// is a multiple of 2^l for every level it serves (l <= 6), the tile maps onto a whole (64 >> l)^2 tile of level l and no
// workgroup needs another's pixels.  Level l + 1 is computed from the level-l BYTES just produced (kept in LDS), so the values
// are those of the level-by-level kernel: the truncating mean of truncated means, not a mean over the 4^l source pixels.
// rows_l = rows >> l (floor division composes), so an odd trailing row / column drops out exactly as in the reference.
constexpr int kTile = 64;
constexpr int kFusedMaxLevels = 7;  // levels 1..6 below a 64 x 64 tile; deeper pyramids finish with the per-level kernel

struct PyramidLevels {
    uint8_t *dst[kFusedMaxLevels];  // [l]: level l (l >= 1); [0]: null, or where to KEEP level 0 when `src` is not the pyramid's own
                                    // level 0 — the frame read straight from pinned host memory (ftk_pyramid_update): the copy engine's
                                    // ~20 us per 300 KB frame become one PCIe read inside this launch
    int32_t n_levels;               // levels to produce here incl. level 0: 2..kFusedMaxLevels
};

// TW x TH: the level-0 tile of a workgroup, 4096 pixels either way.  64 x 64 serves up to seven levels; 256 x 16 serves up to five
// (16 = 2^4) and reads level 0 in 256-byte row pieces instead of 64-byte ones — what matters when the source is pinned HOST
// memory and every piece is a PCIe read (ftk_pyramid_update / ftk_pyramid_build of host images).
template <int TW, int TH>
__global__ void __launch_bounds__(kBlock) pyramid_fused_kernel(const uint8_t *__restrict__ src, int rows, int cols, PyramidLevels lv) {
    static_assert(TW * TH == kTile * kTile && TW % 16 == 0, "4096-pixel tiles, rows loaded 16 bytes per lane");
    __shared__ uint8_t tile[2][TW * TH];  // ping-pong: level l in tile[l & 1], pitch TW >> l
    const int tx = blockIdx.x, ty = blockIdx.y, tid = threadIdx.x;
    const int r0 = ty * TH, c0 = tx * TW;
    constexpr int kSegs = TW / 16;  // 16-byte pieces per tile row
    // level 0 -> LDS: 256 threads x 16 bytes per pass; pixels beyond the image are never read by a valid output
    for (int k = tid; k < TW * TH / 16; k += kBlock) {
        const int r = k / kSegs, seg = (k % kSegs) << 4;
        const int gr = r0 + r, gc = c0 + seg;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (gr < rows) {
            const uint8_t *q = src + (size_t)gr * (size_t)cols + (size_t)gc;
            if (gc + 16 <= cols) {
                __builtin_memcpy(&v, q, 16);  // unaligned 16-byte load
            } else if (gc < cols) {
                uint8_t tmp[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    tmp[i] = (gc + i < cols) ? q[i] : (uint8_t)0;
                }
                __builtin_memcpy(&v, tmp, 16);
            }
        }
        *reinterpret_cast<uint4 *>(&tile[0][r * TW + seg]) = v;
        if (lv.dst[0] != nullptr && gr < rows && gc < cols) {
            uint8_t *o = lv.dst[0] + (size_t)gr * (size_t)cols + (size_t)gc;
            if (gc + 16 <= cols) {
                __builtin_memcpy(o, &v, 16);  // unaligned 16-byte store
            } else {
                for (int i = 0; gc + i < cols; ++i) {
                    o[i] = reinterpret_cast<const uint8_t *>(&v)[i];
                }
            }
        }
    }
    __syncthreads();
    int lrows = rows, lcols = cols;
    for (int l = 1; l < lv.n_levels; ++l) {
        lrows >>= 1;
        lcols >>= 1;
        const int w = TW >> l, h = TH >> l, prev_pitch = TW >> (l - 1);
        const uint8_t *in = tile[(l - 1) & 1];
        uint8_t *out = tile[l & 1];
        const int lr0 = r0 >> l, lc0 = c0 >> l;
        uint8_t *g = lv.dst[l];
        // four horizontally adjacent outputs per thread where the level is wide enough: one 32-bit store
        const int quads = w >= 4 ? w >> 2 : 1, per = w >= 4 ? 4 : w;
        for (int k = tid; k < h * quads; k += kBlock) {
            const int r = k / quads, q = (k - r * quads) * per;
            uint32_t packed = 0;
#pragma unroll 4
            for (int i = 0; i < per; ++i) {
                const uint8_t *t = in + (2 * r) * prev_pitch + 2 * (q + i);
                const uint32_t sum = (uint32_t)t[0] + t[1] + t[prev_pitch] + t[prev_pitch + 1];
                const uint32_t m = sum >> 2;
                out[r * w + q + i] = (uint8_t)m;
                packed |= m << (8 * i);
            }
            const int gr = lr0 + r, gc = lc0 + q;
            if (gr < lrows && gc < lcols) {
                uint8_t *o = g + (size_t)gr * (size_t)lcols + (size_t)gc;
                if (per == 4 && gc + 4 <= lcols && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
                    *reinterpret_cast<uint32_t *>(o) = packed;
                } else {
                    for (int i = 0; i < per && gc + i < lcols; ++i) {
                        o[i] = (uint8_t)(packed >> (8 * i));
                    }
                }
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int f2i(float x) { return (x >= -2147483648.0f && x < 2147483648.0f) ? (int)x : INT_MIN; }
__device__ __forceinline__ int wadd(int a, int b) { return (int)((unsigned)a + (unsigned)b); }

__global__ void __launch_bounds__(64) extract_patch_kernel(DevImage ref, float u, float v, int ex_rows, int ex_cols, float *patch, uint8_t *valid,
                                                           uint32_t *count) {
    const int lane = threadIdx.x;
    const float int_row = floorf(v);
    const float int_col = floorf(u);
    const float dec_row = v - int_row;
    const float dec_col = u - int_col;
    const float w_tl = (1.0f - dec_row) * (1.0f - dec_col);
    const float w_tr = (1.0f - dec_row) * dec_col;
    const float w_bl = dec_row * (1.0f - dec_col);
    const float w_br = dec_row * dec_col;
    const int min_row = wadd(f2i(int_row), -(ex_rows / 2));
    const int min_col = wadd(f2i(int_col), -(ex_cols / 2));
    const int total = ex_rows * ex_cols;
    uint32_t cnt = 0;
    for (int base = 0; base < total; base += 64) {
        const int e = base + lane;
        bool ok = false;
        if (e < total) {
            const int erow = e / ex_cols;
            const int ecol = e - erow * ex_cols;
            const int row = wadd(min_row, erow);
            const int col = wadd(min_col, ecol);
            ok = !(row < 0 || row > ref.rows - 2 || col < 0 || col > ref.cols - 2);
            float value = 0.0f;
            if (ok) {
                const uint8_t *q = ref.data + (long long)row * ref.cols + col;
                value = w_tl * (float)q[0] + w_tr * (float)q[1] + w_bl * (float)q[ref.cols] + w_br * (float)q[ref.cols + 1];
            }
            patch[e] = value;
            valid[e] = ok ? 1 : 0;
        }
        cnt += (uint32_t)__popcll(__ballot(ok));
    }
    if (lane == 0) {
        *count = cnt;
    }
}


// Multi-GPU result exchange (ftk_comm.cpp): the gathered buffer holds `world` packed shards ([u, v] pairs of `cap` features, then
// `cap` status bytes, `shard_bytes` apart); feature i of the global list lives in the shard of the rank whose block contains it
// (blocks as ftk_shard_bounds: the first n % world ranks hold one feature more).
__global__ void __launch_bounds__(kBlock) unpack_klt_shards_kernel(const uint8_t *__restrict__ gathered, int n, int world, int cap, long long shard_bytes,
                                                                   float2 *__restrict__ uv_out, uint8_t *__restrict__ status_out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const int base = n / world, extra = n % world;
    const int big = extra * (base + 1);  // features held by the ranks with base + 1 of them
    int rank, local;
    if (i < big) {
        rank = i / (base + 1);
        local = i - rank * (base + 1);
    } else {
        rank = extra + (i - big) / (base > 0 ? base : 1);
        local = (i - big) - (rank - extra) * base;
    }
    const uint8_t *shard = gathered + shard_bytes * rank;
    uv_out[i] = reinterpret_cast<const float2 *>(shard)[local];
    status_out[i] = shard[(long long)cap * 8 + local];
}


}  // namespace

hipError_t pyramid_downsample_launch(const uint8_t *src, int32_t src_rows, int32_t src_cols, uint8_t *dst, hipStream_t stream) {
    const int dst_rows = src_rows / 2, dst_cols = src_cols / 2;
    if (dst_rows <= 0 || dst_cols <= 0) {
        return hipSuccess;
    }
    const long long groups = (long long)((dst_cols + 3) >> 2) * dst_rows;
    const unsigned blocks = (unsigned)((groups + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(downsample_kernel, dim3(blocks), dim3(kBlock), 0, stream, src, src_cols, dst, dst_rows, dst_cols);
    return hipGetLastError();
}

// Levels 1 .. n_levels - 1 of a pyramid whose level 0 is `level0` (rows x cols): one fused launch for the first six, the
// per-level kernel for anything deeper.  dst[l] / out_rows / out_cols describe level l (entries >= 1 are used).
// `level0_keep` (optional): `level0` is a source OUTSIDE the pyramid (device-visible pinned host memory) and the launch also writes
// it to level0_keep, the pyramid's own level 0.
hipError_t pyramid_build_levels_launch(const uint8_t *level0, int32_t rows, int32_t cols, uint8_t *const *dst, int32_t n_levels, hipStream_t stream,
                                       uint8_t *level0_keep) {
    if (n_levels <= 1) {
        return hipSuccess;
    }
    PyramidLevels lv;
    lv.n_levels = n_levels < kFusedMaxLevels ? n_levels : kFusedMaxLevels;
    for (int l = 0; l < kFusedMaxLevels; ++l) {
        lv.dst[l] = (l >= 1 && l < lv.n_levels) ? dst[l] : nullptr;
    }
    lv.dst[0] = level0_keep;
    // wide tiles (256-byte row pieces) for a source in host memory, when five levels are enough for them (16 rows = 2^4)
    if (level0_keep != nullptr && lv.n_levels <= 5) {
        const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)((rows + 15) / 16));
        hipLaunchKernelGGL((pyramid_fused_kernel<256, 16>), grid, dim3(kBlock), 0, stream, level0, rows, cols, lv);
    } else {
        const dim3 grid((unsigned)((cols + kTile - 1) / kTile), (unsigned)((rows + kTile - 1) / kTile));
        hipLaunchKernelGGL((pyramid_fused_kernel<kTile, kTile>), grid, dim3(kBlock), 0, stream, level0, rows, cols, lv);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        return e;
    }
    for (int l = lv.n_levels; l < n_levels; ++l) {  // (lv.n_levels >= 2: level 1 always comes from the fused launch)
        e = pyramid_downsample_launch(dst[l - 1], rows >> (l - 1), cols >> (l - 1), dst[l], stream);
        if (e != hipSuccess) {
            return e;
        }
    }
    return hipSuccess;
}

hipError_t extract_patch_launch(DevImage ref, float u, float v, int32_t ex_rows, int32_t ex_cols, float *d_patch, uint8_t *d_valid,
                                uint32_t *d_count, hipStream_t stream) {
    hipLaunchKernelGGL(extract_patch_kernel, dim3(1), dim3(64), 0, stream, ref, u, v, ex_rows, ex_cols, d_patch, d_valid, d_count);
    return hipGetLastError();
}

hipError_t unpack_klt_shards_launch(const uint8_t *d_gathered, int32_t n, int32_t world, int32_t cap, int64_t shard_bytes, float *d_uv_out,
                                   uint8_t *d_status_out, hipStream_t stream) {
    if (n <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(unpack_klt_shards_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, d_gathered, n, world, cap,
                       (long long)shard_bytes, reinterpret_cast<float2 *>(d_uv_out), d_status_out);
    return hipGetLastError();
}

// First-use cost out of the callers' timed regions (ftk_warmup): launching this empty kernel makes the runtime load this
// translation unit's code object onto the device, which otherwise happens inside the first real call.
__global__ void pyramid_warm_kernel() {}
hipError_t pyramid_warm(hipStream_t stream) {
    hipLaunchKernelGGL(pyramid_warm_kernel, dim3(1), dim3(64), 0, stream);
    return hipGetLastError();
}

}  // namespace ftk
