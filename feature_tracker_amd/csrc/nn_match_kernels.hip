// nn_match_kernels.hip — everything NNFeatureMatcher::Match does after the network (src/nn_feature_matcher/nn_feature_matcher.cpp:155-216)
// on gfx950: mutual-best matching of a score matrix in ONE read of the matrix, the match-list scatter, and the index -> pixel fill.
//
// The contract is the scalar loops' own: per column the first argmax over the rows (:188-199), per row the first
// argmax over the columns (:201-210), both by "start at index 0, replace on a strict >".  It is met with comparisons only.  A score s
// at index k becomes the unsigned key
//     nn_order(s, k) << 32 | ~k
// where nn_order is the usual order-preserving map of a float onto uint32 with three amendments: -0 is folded onto +0 (they tie, so the
// lower index must win), a NaN at index 0 maps to the top value (nothing compares greater than NaN: it keeps its column / row), and a
// NaN anywhere else maps to 0, below -inf (it never compares greater).  The greatest key is then exactly the loop's answer — greatest
// score, lowest index among equals — and keys merge in any order: across the lanes of a wave (shuffles), the waves of a workgroup
// (LDS) and the tiles of the grid (64-bit vector atomicMax on row_key / col_key, which hold 0 = "empty" between calls).
#include <hip/hip_runtime.h>

#include "ftk_device.h"
#include "match_plan.h"

namespace ftk {

namespace {

constexpr int kBlock = kNnBlock;
constexpr int kWaves = kBlock / kWave;
constexpr int kInFlight = 4;  // row segments a wave loads before it works on them
static_assert(kNnTileCols == 4 * kWave, "a lane owns four consecutive columns of the tile");
static_assert(kNnTileRowsMin == kWaves * kInFlight && kNnTileRowsMax <= kBlock, "tile rows: whole rounds of the waves; one thread per row merges");

__device__ __forceinline__ uint32_t nn_order(float s, uint32_t index) {
    if (s != s) {
        return index == 0 ? 0xFFFFFFFFu : 0u;
    }
    const uint32_t u = s == 0.0f ? 0u : __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The score a key's upper word stands for (the row maximum the threshold test reads; -0 comes back as +0, which compares alike).
__device__ __forceinline__ float nn_score_of(uint32_t ordered) {
    if (ordered == 0xFFFFFFFFu) {
        return __uint_as_float(0x7FC00000u);
    }
    return __uint_as_float((ordered & 0x80000000u) ? (ordered ^ 0x80000000u) : ~ordered);
}

__device__ __forceinline__ unsigned long long nn_key(float s, uint32_t index) { return ((unsigned long long)nn_order(s, index) << 32) | (uint32_t)~index; }

__device__ __forceinline__ unsigned long long key_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

__device__ __forceinline__ unsigned long long wave_key_max(unsigned long long k) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)k, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), off);
        k = key_max(k, ((unsigned long long)hi << 32) | lo);
    }
    return k;
}

// One tile: wave w takes the tile's rows w, w + 4, ... kInFlight at a time; a lane keeps the running keys of its four columns in
// registers and the row's key goes through the wave reduction into LDS.  Out-of-range elements are skipped (their keys stay 0).
template <bool VEC4>
__global__ void __launch_bounds__(kBlock) nn_mutual_kernel(const NnMatchParams p) {
    __shared__ unsigned long long row_keys[kNnTileRowsMax];
    __shared__ unsigned long long col_keys[kWaves][kNnTileCols];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int32_t ct = (int32_t)(blockIdx.x % (uint32_t)p.col_tiles), rt = (int32_t)(blockIdx.x / (uint32_t)p.col_tiles);
    const int32_t b = (int32_t)blockIdx.y;
    const int32_t c0 = ct * kNnTileCols + lane * 4;  // < n_cur + kNnTileCols: no overflow (n_ref + n_cur < 2^31)
    const int32_t r0 = rt * p.tile_rows;
    const float *base = p.scores + (int64_t)b * p.batch_stride;
    const int32_t cols_here = p.n_cur - c0;  // columns of this lane that exist: <= 0 none, >= 4 all
    unsigned long long ck[4] = {0ull, 0ull, 0ull, 0ull};
    for (int32_t rr = wave; rr < p.tile_rows; rr += kWaves * kInFlight) {
        float v[kInFlight][4];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const int32_t r = r0 + rr + k * kWaves;
            const float *row = base + (int64_t)r * p.row_stride + c0;
            if (r < p.n_ref && cols_here >= 4 && VEC4) {
                const float4 q = *reinterpret_cast<const float4 *>(row);
                v[k][0] = q.x, v[k][1] = q.y, v[k][2] = q.z, v[k][3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[k][e] = (r < p.n_ref && e < cols_here) ? row[e] : 0.0f;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const int32_t r = r0 + rr + k * kWaves;
            if (r0 + rr + k * kWaves - wave >= p.n_ref) {  // wave-uniform: no wave of this round has the row
                break;
            }
            unsigned long long rk = 0ull;
            if (r < p.n_ref) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (e < cols_here) {
                        ck[e] = key_max(ck[e], nn_key(v[k][e], (uint32_t)r));
                        rk = key_max(rk, nn_key(v[k][e], (uint32_t)(c0 + e)));
                    }
                }
            }
            rk = wave_key_max(rk);
            if (lane == 0) {
                row_keys[rr + k * kWaves] = rk;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        col_keys[wave][lane * 4 + e] = ck[e];
    }
    __syncthreads();
    {
        const int32_t c = ct * kNnTileCols + (int32_t)threadIdx.x;
        if (c < p.n_cur) {
            unsigned long long k = col_keys[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) {
                k = key_max(k, col_keys[w][threadIdx.x]);
            }
            atomicMax(&p.col_key[(int64_t)b * p.n_cur + c], k);
        }
        const int32_t r = r0 + (int32_t)threadIdx.x;
        if ((int32_t)threadIdx.x < p.tile_rows && r < p.n_ref) {
            atomicMax(&p.row_key[(int64_t)b * p.n_ref + r], row_keys[threadIdx.x]);
        }
    }
}

// Threshold (:211), mutual check (:212), outputs; every key goes back to 0.  A thread empties its own row key; the column keys are
// read by other workgroups, so the last workgroup to finish empties them (and the counter) once every reader has its value.
__global__ void __launch_bounds__(kBlock) nn_mutual_epilogue_kernel(const NnMatchParams p) {
    __shared__ bool last;
    const int64_t rows = (int64_t)p.batch * p.n_ref;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t < rows) {
        const int32_t b = (int32_t)(t / p.n_ref), i = (int32_t)(t % p.n_ref);
        const unsigned long long rk = p.row_key[t];
        const uint32_t j = ~(uint32_t)rk;
        const float best = nn_score_of((uint32_t)(rk >> 32));
        const unsigned long long ck = j < (uint32_t)p.n_cur ? p.col_key[(int64_t)b * p.n_cur + j] : 0ull;  // (always in range on clean keys)
        const bool matched = !(best < p.min_score) && ~(uint32_t)ck == (uint32_t)i;
        p.match_index[t] = matched ? (int32_t)j : -1;
        p.status[t] = matched ? FTK_TRACKED : FTK_LARGE_RESIDUAL;
        p.row_key[t] = 0ull;
    }
    __syncthreads();  // every thread of the workgroup has consumed its column key
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(p.done, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (last) {
        const int64_t cols = (int64_t)p.batch * p.n_cur;
        for (int64_t c = threadIdx.x; c < cols; c += kBlock) {
            p.col_key[c] = 0ull;
        }
        if (threadIdx.x == 0) {
            *p.done = 0u;
        }
    }
}

// List mode (:166-174): row k is applied iff both indices are in range; the applied row with the largest k wins its idx_ref.
__global__ void __launch_bounds__(kBlock) nn_match_list_kernel(const long long *matches, int32_t n_matches, int32_t n_ref, int32_t n_cur,
                                                               unsigned long long *row_key) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < n_matches) {
        const long long idx_ref = matches[2 * k], idx_cur = matches[2 * k + 1];
        const long long ref_bound = n_ref < n_cur ? n_ref : n_cur;
        if (idx_ref >= 0 && idx_ref < ref_bound && idx_cur >= 0 && idx_cur < n_cur) {
            atomicMax(&row_key[idx_ref], ((unsigned long long)(k + 1) << 32) | (uint32_t)idx_cur);
        }
    }
}

__global__ void __launch_bounds__(kBlock) nn_list_epilogue_kernel(unsigned long long *row_key, int32_t n_ref, int32_t *match_index, uint8_t *status) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n_ref) {
        const unsigned long long key = row_key[i];
        match_index[i] = key ? (int32_t)(uint32_t)key : -1;
        status[i] = key ? FTK_TRACKED : FTK_LARGE_RESIDUAL;
        row_key[i] = 0ull;
    }
}

// matched_uv (n_cur entries, :157) as a gather: entry t is cur_uv[match_index[t]] where reference row t exists and is matched, else
// cur_uv[t].  matched_uv must not alias cur_uv.
__global__ void __launch_bounds__(kBlock) nn_fill_pixels_kernel(const int32_t *match_index, int32_t n_ref, const float *cur_uv, int32_t n_cur,
                                                                float *matched_uv) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t < n_cur) {
        int64_t src = t;
        if (t < n_ref) {
            const int32_t j = match_index[t];
            if (j >= 0 && j < n_cur) {
                src = j;
            }
        }
        matched_uv[2 * t] = cur_uv[2 * src];
        matched_uv[2 * t + 1] = cur_uv[2 * src + 1];
    }
}

__global__ void nn_match_warm_kernel() {}

dim3 blocks_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

}  // namespace

hipError_t nn_match_scores_launch(const NnMatchPlan &plan, const NnMatchParams &p, hipStream_t stream) {
    if (plan.vec4) {
        hipLaunchKernelGGL(nn_mutual_kernel<true>, plan.grid, plan.block, 0, stream, p);
    } else {
        hipLaunchKernelGGL(nn_mutual_kernel<false>, plan.grid, plan.block, 0, stream, p);
    }
    hipLaunchKernelGGL(nn_mutual_epilogue_kernel, plan.epilogue_grid, dim3(kBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t nn_match_list_launch(const long long *matches, int32_t n_matches, int32_t n_ref, int32_t n_cur, unsigned long long *row_key,
                                int32_t *match_index, uint8_t *status, hipStream_t stream) {
    if (n_matches > 0) {
        hipLaunchKernelGGL(nn_match_list_kernel, blocks_for(n_matches), dim3(kBlock), 0, stream, matches, n_matches, n_ref, n_cur, row_key);
    }
    hipLaunchKernelGGL(nn_list_epilogue_kernel, blocks_for(n_ref), dim3(kBlock), 0, stream, row_key, n_ref, match_index, status);
    return hipGetLastError();
}

hipError_t nn_fill_pixels_launch(const int32_t *match_index, int32_t n_ref, const float *cur_uv, int32_t n_cur, float *matched_uv, hipStream_t stream) {
    hipLaunchKernelGGL(nn_fill_pixels_kernel, blocks_for(n_cur), dim3(kBlock), 0, stream, match_index, n_ref, cur_uv, n_cur, matched_uv);
    return hipGetLastError();
}

hipError_t nn_match_warm(hipStream_t stream) {
    hipLaunchKernelGGL(nn_match_warm_kernel, dim3(1), dim3(64), 0, stream);
    return hipGetLastError();
}

}  // namespace ftk
