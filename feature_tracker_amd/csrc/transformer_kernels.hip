// transformer_kernels.hip — LightGlue's transformer layer on gfx950 (TransformerLayer): the self block on both descriptor
// sets and the cross block in both directions, 12 launches, with no copy to the host.
//
//  * linear_kernel: a Linear over the M + N rows of both sets as one GEMM on the f32-input matrix cores (mfma_tile_gemm.h's tile_gemm,
//    a k-ordered fmaf chain from the bias).  The input is one row segment or two read in place of their cat; the epilogue is none, the
//    residual add, or the rotary encoding.  For the rotary form a lane's column tiles 2 u and 2 u + 1 hold outputs 2 j and 2 j + 1 of
//    one pair, so a pair's two outputs meet in one lane.  Outputs may be split into planes (q | k | v).
//  * attention_kernel: a wave owns 32 query rows of one head and 32 kOut of its output columns.  It walks the key tiles three times
//    and recomputes s = q k^T on the matrix cores each time, so the [h, M, N] scores never reach memory: the maximum m; the 64 partial
//    sums of exp_c(s - m) and their xor tree, l; then p = exp_c(s - m) / l, which leaves the matrix core in its D layout, passes
//    through LDS and comes back as an A operand of p v, accumulated in ONE accumulator over ascending keys.  blockIdx.z is the set
//    (self block) or the direction (cross block).
//  * layernorm_gelu_kernel: one wave per row, in place.
//
// Every float operation is written out (fmaf, __f*_rn); with -ffp-contract=off the results are bit-identical to the scalar restatement
// tests/transformer_ref.c.  Out-of-range rows and columns of a tile read row 0 and are never stored; every index is 64-bit; no address
// depends on data.
#include "mfma_tile_gemm.h"
#include "raft_math.h"
#include "transformer_plan.h"

namespace ftk {
namespace {

static_assert(kLinearTileCols == 32 * kColTiles && kAttnKeyTile == 32 * kColTiles, "tile_gemm's 4 column tiles");

constexpr float kSqrtHalf = 0x1.6a09e6p-1f;  // (float)M_SQRT1_2

// Whether any of the rows [begin, end) of the two sets laid one behind the other (the second from rows0) is in front of its set's
// live count.
__device__ __forceinline__ bool any_live_row(int begin, int end, int rows0, int live0, int live1) {
    const int begin1 = (begin > rows0 ? begin : rows0) - rows0;
    return begin < live0 || (end > rows0 && begin1 < live1);
}

template <bool kVec>
__global__ void __launch_bounds__(64 * kLinearWaves) linear_kernel(const LinearParams p) {
    const int lane = threadIdx.x & 63, j = lane & 31, kh = lane >> 5;
    const int rows = p.rows, rows0 = p.rows0, outs = p.outs;
    const int r0 = (blockIdx.x * kLinearWaves + (threadIdx.x >> 6)) * 32;  // wave-uniform
    if (r0 >= rows) {
        return;
    }
    if (p.gate) {  // the adaptive pass: a stopped layer, or 32 rows that are all pruned (wave-uniform; this kernel has no barrier)
        if (p.gate[0] != 0 || !any_live_row(r0, r0 + 32 < rows ? r0 + 32 : rows, rows0, valid_count(p.live0, rows0), valid_count(p.live1, rows - rows0))) {
            return;
        }
    }
    const int o0 = blockIdx.y * kLinearTileCols;
    const bool rotary = p.epilogue == kLinearRotary;
    const int ra = r0 + j < rows ? r0 + j : 0;
    const float *a = ra < rows0 ? p.a0 + (size_t)ra * p.ka : p.a1 + (size_t)(ra - rows0) * p.ka;
    const size_t k_all = (size_t)p.ka + (size_t)p.kb;
    const float *b[kColTiles];
    int col[kColTiles];
    f32x16 acc[kColTiles];
#pragma unroll
    for (int t = 0; t < kColTiles; ++t) {
        col[t] = rotary ? o0 + 64 * (t >> 1) + 2 * j + (t & 1) : o0 + 32 * t + j;
        const int ob = col[t] < outs ? col[t] : 0;
        b[t] = p.w + (size_t)ob * k_all;
        const float bias = p.bias[ob];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[t][r] = bias;
        }
    }
    tile_gemm<kVec>(a, b, p.ka, 1.0f, kh, acc);
    if (p.b) {
        const float *a2 = p.b + (size_t)ra * p.kb;
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            b[t] += p.ka;
        }
        tile_gemm<kVec>(a2, b, p.kb, 1.0f, kh, acc);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = r0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (row >= rows) {
            continue;
        }
        const bool first = row < rows0;
        const size_t lr = (size_t)(first ? row : row - rows0), set_rows = (size_t)(first ? rows0 : rows - rows0);
        float *out = first ? p.out0 : p.out1;
        float y[kColTiles];
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            y[t] = acc[t][r];
        }
        if (rotary) {
            const float *enc = first ? p.enc0 : p.enc1;
#pragma unroll
            for (int u = 0; u < kColTiles / 2; ++u) {
                const int oe = col[2 * u];
                if (oe < p.rotary_outs) {
                    const size_t el = (size_t)((oe % p.plane_cols) % p.head_dim);
                    const float *cs = enc + lr * p.head_dim + el, *sn = enc + (set_rows + lr) * p.head_dim + el;
                    const float te = y[2 * u], to = y[2 * u + 1];
                    y[2 * u] = __fadd_rn(__fmul_rn(te, cs[0]), __fmul_rn(-to, sn[0]));
                    y[2 * u + 1] = __fadd_rn(__fmul_rn(to, cs[1]), __fmul_rn(te, sn[1]));
                }
            }
        }
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            const int o = col[t];
            if (o >= outs) {
                continue;
            }
            float v = y[t];
            if (p.epilogue == kLinearResidual) {
                v = __fadd_rn((first ? p.x0 : p.x1)[lr * outs + o], v);
            }
            const int plane = o / p.plane_cols, c = o % p.plane_cols;
            out[(size_t)plane * p.plane_stride + lr * p.plane_cols + c] = v;
        }
    }
}

// s of one key tile: acc[t][r] = the fmaf chain over the head's channels of (q pre)(k pre), for row (r & 3) + 8 (r >> 2) + 4 kh of the
// wave's 32 queries and key key0 + 32 t + (lane & 31); a key at or behind rows_k reads key 0.
template <bool kVec>
__device__ __forceinline__ void score_tile(const float *qrow, const float *khead, int key0, int rows_k, int dim, int head_dim, float pre, int j, int kh,
                                           f32x16 (&acc)[kColTiles]) {
    const float *b[kColTiles];
#pragma unroll
    for (int t = 0; t < kColTiles; ++t) {
        const int key = key0 + 32 * t + j;
        b[t] = khead + (size_t)(key < rows_k ? key : 0) * dim;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[t][r] = 0.0f;
        }
    }
    tile_gemm<kVec>(qrow, b, head_dim, pre, kh, acc);
}

template <bool kVec, int kOut>
__global__ void __launch_bounds__(kAttnThreads) attention_kernel(const AttentionParams p, int splits) {
    __shared__ float tile[32 * kAttnLdsStride];
    const int lane = threadIdx.x, j = lane & 31, kh = lane >> 5;
    const bool z = blockIdx.z != 0;
    const int rows_q = z ? p.prob[1].rows_q : p.prob[0].rows_q, rows_k = z ? p.prob[1].rows_k : p.prob[0].rows_k;
    const int i0 = blockIdx.x * 32;  // block-uniform, as all control flow below
    if (i0 >= rows_q) {
        return;
    }
    if (p.gate) {  // the adaptive pass: a stopped layer, or 32 queries that are all pruned (before the first load and the first barrier)
        if (p.gate[0] != 0 || i0 >= valid_count(z ? p.prob[1].live_q : p.prob[0].live_q, rows_q)) {
            return;
        }
    }
    const float *q = z ? p.prob[1].q : p.prob[0].q, *k = z ? p.prob[1].k : p.prob[0].k, *v = z ? p.prob[1].v : p.prob[0].v;
    float *out = z ? p.prob[1].out : p.prob[0].out;
    const int n = valid_count(z ? p.prob[1].count : p.prob[0].count, rows_k);
    const int dim = p.dim, dh = p.head_dim;
    const int head = blockIdx.y / splits, split = blockIdx.y % splits;
    const size_t head_at = (size_t)head * dh;
    const float *qrow = q + (size_t)(i0 + j < rows_q ? i0 + j : 0) * dim + head_at;
    const float *khead = k + head_at;
    const float pre = p.pre, post = p.post;
    const float ninf = -__builtin_huge_valf();
    const int tiles_n = (n + kAttnKeyTile - 1) / kAttnKeyTile;
    f32x16 acc[kColTiles];

    // 1. m: the first entry, and the greatest entry that is no NaN
    float m[16], first[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        m[r] = ninf;
        first[r] = 0.0f;
    }
    for (int kt = 0; kt < tiles_n; ++kt) {
        score_tile<kVec>(qrow, khead, kt * kAttnKeyTile, rows_k, dim, dh, pre, j, kh, acc);
        if (kt == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                first[r] = __shfl(__fmul_rn(acc[0][r], post), lane & 32);
            }
        }
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            const bool valid = kt * kAttnKeyTile + 32 * t + j < n;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float x = __fmul_rn(acc[t][r], post);
                if (valid && x > m[r]) {
                    m[r] = x;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        m[r] = scan_maximum(first[r], xor_greatest<16>(m[r]));
    }

    // 2. l: the partial sums = key (mod 64) live in lane (key & 31) as two accumulators; the xor tree's first round adds those two
    float l[16];
    {
        float part[16][2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            part[r][0] = part[r][1] = 0.0f;
        }
        for (int kt = 0; kt < tiles_n; ++kt) {
            score_tile<kVec>(qrow, khead, kt * kAttnKeyTile, rows_k, dim, dh, pre, j, kh, acc);
#pragma unroll
            for (int t = 0; t < kColTiles; ++t) {
                const bool valid = kt * kAttnKeyTile + 32 * t + j < n;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float e = exp_c(__fsub_rn(__fmul_rn(acc[t][r], post), m[r]));
                    if (valid) {
                        part[r][t & 1] = __fadd_rn(part[r][t & 1], e);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            l[r] = xor_sum<16>(__fadd_rn(part[r][0], part[r][1]));  // (round 32 is the add of the lane's own two partials)
        }
    }

    // 3. p v over ascending keys, in one accumulator per output
    f32x16 res[kOut];
    int dcol[kOut];
    bool dvalid[kOut];
#pragma unroll
    for (int u = 0; u < kOut; ++u) {
        dcol[u] = (split * kOut + u) * 32 + j;
        dvalid[u] = dcol[u] < dh;
        dcol[u] = dvalid[u] ? dcol[u] : 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            res[u][r] = 0.0f;
        }
    }
    const float *vhead = v + head_at;
    for (int kt = 0; kt < tiles_n; ++kt) {
        score_tile<kVec>(qrow, khead, kt * kAttnKeyTile, rows_k, dim, dh, pre, j, kh, acc);
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            const int key0 = kt * kAttnKeyTile + 32 * t;
            if (key0 >= n) {
                continue;
            }
            const bool valid = key0 + j < n;
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __fdiv_rn(exp_c(__fsub_rn(__fmul_rn(acc[t][r], post), m[r])), l[r]);
                tile[((r & 3) + 8 * (r >> 2) + 4 * kh) * kAttnLdsStride + j] = valid ? pv : -0.0f;
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int key = key0 + 2 * s + kh;
                const float a = tile[j * kAttnLdsStride + 2 * s + kh];
                const float *vrow = vhead + (size_t)(key < rows_k ? key : 0) * dim;
#pragma unroll
                for (int u = 0; u < kOut; ++u) {
                    const float loaded = vrow[dcol[u]];
                    const float bv = key < n && dvalid[u] ? loaded : 0.0f;
                    res[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, res[u], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (row >= rows_q) {
            continue;
        }
#pragma unroll
        for (int u = 0; u < kOut; ++u) {
            if (dvalid[u]) {
                out[(size_t)row * dim + head_at + dcol[u]] = res[u][r];
            }
        }
    }
}

__global__ void __launch_bounds__(kNormThreads) layernorm_gelu_kernel(const NormParams p) {
    const int lane = threadIdx.x, cols = p.cols;
    if (p.gate) {  // the adaptive pass: a stopped layer or a pruned row
        const int row = blockIdx.x;
        if (p.gate[0] != 0 || !any_live_row(row, row + 1, p.rows0, valid_count(p.live0, p.rows0), valid_count(p.live1, p.n_rows - p.rows0))) {
            return;
        }
    }
    float *x = p.rows + (size_t)blockIdx.x * cols;
    const float n = (float)cols;
    float s1 = 0.0f;
    for (int c = lane; c < cols; c += 64) {
        s1 = __fadd_rn(s1, x[c]);
    }
    const float mean = __fdiv_rn(xor_sum(s1), n);
    float s2 = 0.0f;
    for (int c = lane; c < cols; c += 64) {
        const float d = __fsub_rn(x[c], mean);
        s2 = fmaf(d, d, s2);
    }
    const float var = __fdiv_rn(xor_sum(s2), n);
    const float rstd = __fdiv_rn(1.0f, sqrtf(__fadd_rn(var, 1e-5f)));  // (correctly rounded by the build's flags; __fsqrt_rn is the native one)
    for (int c = lane; c < cols; c += 64) {
        const float d = __fsub_rn(x[c], mean);
        const float y = fmaf(__fmul_rn(d, rstd), p.gamma[c], p.beta[c]);
        x[c] = __fmul_rn(__fmul_rn(0.5f, y), __fadd_rn(1.0f, erf_c(__fmul_rn(y, kSqrtHalf))));
    }
}

template <bool kVec>
void launch_attention(const TransformerPlan &plan, const AttentionParams &p, int splits, hipStream_t stream) {
    const dim3 grid(plan.attn_grid_x, plan.attn_grid_y, plan.attn_grid_z), block(kAttnThreads);
    if (plan.attn_out_tiles == 1) {
        hipLaunchKernelGGL((attention_kernel<kVec, 1>), grid, block, 0, stream, p, splits);
    } else if (plan.attn_out_tiles == 2) {
        hipLaunchKernelGGL((attention_kernel<kVec, 2>), grid, block, 0, stream, p, splits);
    } else {
        hipLaunchKernelGGL((attention_kernel<kVec, 4>), grid, block, 0, stream, p, splits);
    }
}

}  // namespace

hipError_t linear_launch(const LinearParams &p, bool vec, uint32_t grid_x, uint32_t grid_y, hipStream_t stream) {
    const dim3 grid(grid_x, grid_y);
    if (vec) {
        hipLaunchKernelGGL(linear_kernel<true>, grid, dim3(64 * kLinearWaves), 0, stream, p);
    } else {
        hipLaunchKernelGGL(linear_kernel<false>, grid, dim3(64 * kLinearWaves), 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t attention_launch(const TransformerPlan &plan, const AttentionParams &p, hipStream_t stream) {
    const int splits = (p.head_dim + 32 * plan.attn_out_tiles - 1) / (32 * plan.attn_out_tiles);
    if (plan.vec_attn) {
        launch_attention<true>(plan, p, splits, stream);
    } else {
        launch_attention<false>(plan, p, splits, stream);
    }
    return hipGetLastError();
}

hipError_t layernorm_gelu_launch(const NormParams &p, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(layernorm_gelu_kernel, dim3(blocks), dim3(kNormThreads), 0, stream, p);
    return hipGetLastError();
}

}  // namespace ftk
