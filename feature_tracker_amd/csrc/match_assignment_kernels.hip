// match_assignment_kernels.hip — LightGlue's assignment head on gfx950 (MatchAssignment): from two descriptor sets to the
// [M + 1][N + 1] log-assignment tensor that NNFeatureMatcher reads, with no copy to the host.
//
//  * match_project_kernel: both descriptor sets through final_proj and matchability as one GEMM on the f32-input matrix cores
//    (v_mfma_f32_32x32x2_f32, corr_build_kernel's k order): rows are the M + N descriptors, columns the D outputs and, as column D, z.  The
//    accumulators start from the bias; the epilogue divides the D outputs by q.
//  * match_similarity_kernel: sim = md0 md1^T, the same GEMM from +0, written straight into the output tensor.  Without weights it reads
//    the descriptors themselves and multiplies each element by `scale` as it is loaded.
//  * match_normalise_kernel: one wave per row (lane l owns columns l, l + 64, ...), then one wave per 16 columns.  A column wave reads
//    tiles of 64 rows as 16 loads of 4 rows x 16 columns, passes the exponentials through LDS and takes them back transposed, so that
//    lane l owns rows l, l + 64, ... of all 16 columns: the stated partial sums, whatever the launch shape.  Both write log-sum-exp
//    and, with weights, ls(z) and ls(-z).
//  * match_finish_kernel: in place, every entry of the [M + 1][N + 1] tensor: the double log-softmax, the dustbins, the -inf fill.
//
// Every float operation is written out (fmaf, __f*_rn); with -ffp-contract=off the results are bit-identical to the scalar restatement
// tests/match_assignment_ref.c.  Out-of-range rows and columns of a tile read row 0 and are never stored.
#include "match_assignment_plan.h"
#include "mfma_tile_gemm.h"
#include "raft_math.h"

namespace ftk {
namespace {

static_assert(kAssignGemmTileCols == 32 * kColTiles, "tile_gemm's 4 column tiles");

template <bool kVec>
__global__ void __launch_bounds__(64 * kAssignGemmWaves) match_project_kernel(const MatchAssignmentParams p) {
    const int lane = threadIdx.x & 63, j = lane & 31, kh = lane >> 5;
    const int rows = p.rows0 + p.rows1, dim = p.dim;
    const int r0 = (blockIdx.x * kAssignGemmWaves + (threadIdx.x >> 6)) * 32;  // wave-uniform
    if (r0 >= rows) {
        return;
    }
    const int o0 = blockIdx.y * kAssignGemmTileCols;
    const int ra = r0 + j < rows ? r0 + j : 0;
    const float *a = ra < p.rows0 ? p.desc0 + (size_t)ra * dim : p.desc1 + (size_t)(ra - p.rows0) * dim;
    const float *b[kColTiles];
    f32x16 acc[kColTiles];
#pragma unroll
    for (int t = 0; t < kColTiles; ++t) {
        const int o = o0 + 32 * t + j;
        const int ob = o <= dim ? o : 0;
        b[t] = p.weights + (size_t)ob * dim;
        const float bias = p.bias[ob];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[t][r] = bias;
        }
    }
    tile_gemm<kVec>(a, b, dim, 1.0f, kh, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = r0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (row >= rows) {
            continue;
        }
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            const int o = o0 + 32 * t + j;
            if (o < dim) {
                p.md[(size_t)row * dim + o] = __fdiv_rn(acc[t][r], p.q);
            } else if (o == dim) {
                p.z[row] = acc[t][r];
            }
        }
    }
}

template <bool kVec>
__global__ void __launch_bounds__(64 * kAssignGemmWaves) match_similarity_kernel(const MatchAssignmentParams p) {
    const int lane = threadIdx.x & 63, j = lane & 31, kh = lane >> 5;
    const int dim = p.dim;
    const int i0 = (blockIdx.x * kAssignGemmWaves + (threadIdx.x >> 6)) * 32;  // wave-uniform
    if (i0 >= p.rows0) {
        return;
    }
    const int j0 = blockIdx.y * kAssignGemmTileCols;
    const bool projected = p.weights != nullptr;
    const float *src0 = projected ? p.md : p.desc0;
    const float *src1 = projected ? p.md + (size_t)p.rows0 * dim : p.desc1;
    const float *a = src0 + (size_t)(i0 + j < p.rows0 ? i0 + j : 0) * dim;
    const float *b[kColTiles];
    f32x16 acc[kColTiles];
#pragma unroll
    for (int t = 0; t < kColTiles; ++t) {
        const int col = j0 + 32 * t + j;
        b[t] = src1 + (size_t)(col < p.rows1 ? col : 0) * dim;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[t][r] = 0.0f;
        }
    }
    tile_gemm<kVec>(a, b, dim, projected ? 1.0f : p.scale, kh, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (row >= p.rows0) {
            continue;
        }
        float *out = p.scores + (size_t)row * p.row_stride;
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            const int col = j0 + 32 * t + j;
            if (col < p.rows1) {
                out[col] = acc[t][r];
            }
        }
    }
}

__global__ void __launch_bounds__(kAssignNormThreads) match_normalise_kernel(const MatchAssignmentParams p, uint32_t row_blocks) {
    __shared__ float tile[64 * kAssignNormLdsStride];
    const int lane = threadIdx.x;
    const int n0 = valid_count(p.count0, p.rows0), n1 = valid_count(p.count1, p.rows1);  // block-uniform, as all control flow below
    const float ninf = -__builtin_huge_valf();
    if (blockIdx.x < row_blocks) {
        const int i = blockIdx.x;
        if (i >= n0) {
            return;
        }
        if (p.weights && lane == 0) {
            const float z = p.z[i];
            p.ls0[i] = log_sigmoid_c(z);
            p.ls0[p.rows0 + i] = log_sigmoid_c(-z);
        }
        if (n1 == 0) {
            return;
        }
        const float *row = p.scores + (size_t)i * p.row_stride;
        float greatest = ninf;
        for (int c = lane; c < n1; c += 64) {
            const float x = row[c];
            if (x > greatest) {
                greatest = x;
            }
        }
        greatest = xor_greatest(greatest);
        const float m = scan_maximum(row[0], greatest);
        float sum = 0.0f;
        for (int c = lane; c < n1; c += 64) {
            sum = __fadd_rn(sum, exp_c(__fsub_rn(row[c], m)));
        }
        sum = xor_sum(sum);
        if (lane == 0) {
            p.lse_row[i] = __fadd_rn(m, log_c(sum));
        }
        return;
    }
    const int c0 = (int)(blockIdx.x - row_blocks) * kAssignNormCols;
    if (c0 >= n1) {
        return;
    }
    const int cc = lane & (kAssignNormCols - 1), g = lane / kAssignNormCols;  // this lane loads column c0 + cc of rows 4 t + g
    constexpr int kGroups = 64 / kAssignNormCols;
    const bool owner = g == 0 && c0 + cc < n1;
    const int col = min(c0 + cc, n1 - 1);  // a lane behind the last valid column computes that column again and stores nothing
    if (p.weights && owner) {
        const float z = p.z[p.rows0 + col];
        p.ls1[col] = log_sigmoid_c(z);
        p.ls1[p.rows1 + col] = log_sigmoid_c(-z);
    }
    if (n0 == 0) {
        return;
    }
    const float *src = p.scores + col;
    float greatest = ninf;
    for (int i = g; i < n0; i += kGroups) {
        const float x = src[(size_t)i * p.row_stride];
        if (x > greatest) {
            greatest = x;
        }
    }
    greatest = xor_greatest<32, kAssignNormCols>(greatest);
    const float m = scan_maximum(src[0], greatest);
    float sums[kAssignNormCols];  // of column c0 + k over the rows = lane (mod 64)
#pragma unroll
    for (int k = 0; k < kAssignNormCols; ++k) {
        sums[k] = 0.0f;
    }
    for (int i0 = 0; i0 < n0; i0 += 64) {
#pragma unroll
        for (int t = 0; t < 64 / kGroups; ++t) {
            const int r = kGroups * t + g;
            float e = 0.0f;
            if (i0 + r < n0) {
                e = exp_c(__fsub_rn(src[(size_t)(i0 + r) * p.row_stride], m));
            }
            tile[r * kAssignNormLdsStride + cc] = e;
        }
        __syncthreads();
        if (i0 + lane < n0) {
#pragma unroll
            for (int k = 0; k < kAssignNormCols; ++k) {
                sums[k] = __fadd_rn(sums[k], tile[lane * kAssignNormLdsStride + k]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kAssignNormCols; ++k) {
        sums[k] = xor_sum(sums[k]);
    }
    float sum = sums[0];
#pragma unroll
    for (int k = 1; k < kAssignNormCols; ++k) {
        sum = cc == k ? sums[k] : sum;
    }
    if (owner) {
        p.lse_col[col] = __fadd_rn(m, log_c(sum));
    }
}

__global__ void __launch_bounds__(kAssignFinishThreads) match_finish_kernel(const MatchAssignmentParams p) {
    const int j = blockIdx.x * kAssignFinishThreads + threadIdx.x;
    const int M = p.rows0, N = p.rows1;
    if (j > N) {
        return;
    }
    const int n0 = valid_count(p.count0, M), n1 = valid_count(p.count1, N);
    const bool certain = p.weights != nullptr;
    const float ninf = -__builtin_huge_valf();
    const bool col_valid = j < n1;
    const float lse_col = col_valid && n0 > 0 ? p.lse_col[j] : 0.0f;
    const float ls1 = certain && col_valid ? p.ls1[j] : 0.0f;
    const float bin1 = certain && col_valid ? p.ls1[N + j] : ninf;
    for (int k = 0; k < kAssignFinishRows; ++k) {
        const int i = blockIdx.y * kAssignFinishRows + k;
        if (i > M) {
            return;
        }
        float *row = p.scores + (size_t)i * p.row_stride;
        float v = ninf;
        if (i == M) {
            v = j == N ? 0.0f : bin1;
        } else if (i < n0) {
            if (j == N) {
                v = certain ? p.ls0[M + i] : ninf;
            } else if (col_valid) {
                const float s = row[j];
                v = __fadd_rn(__fsub_rn(s, p.lse_row[i]), __fsub_rn(s, lse_col));
                if (certain) {
                    v = __fadd_rn(v, __fadd_rn(p.ls0[i], ls1));
                }
            }
        }
        row[j] = v;
    }
}

}  // namespace

hipError_t match_assignment_launch(const MatchAssignmentPlan &plan, const MatchAssignmentParams &p, hipStream_t stream) {
    const dim3 gemm_block(64 * kAssignGemmWaves);
    if (plan.project_grid_x > 0) {
        const dim3 grid(plan.project_grid_x, plan.project_grid_y);
        if (plan.vec) {
            hipLaunchKernelGGL(match_project_kernel<true>, grid, gemm_block, 0, stream, p);
        } else {
            hipLaunchKernelGGL(match_project_kernel<false>, grid, gemm_block, 0, stream, p);
        }
    }
    const dim3 sim_grid(plan.sim_grid_x, plan.sim_grid_y);
    if (plan.vec) {
        hipLaunchKernelGGL(match_similarity_kernel<true>, sim_grid, gemm_block, 0, stream, p);
    } else {
        hipLaunchKernelGGL(match_similarity_kernel<false>, sim_grid, gemm_block, 0, stream, p);
    }
    hipLaunchKernelGGL(match_normalise_kernel, dim3(plan.norm_row_blocks + plan.norm_col_blocks), dim3(kAssignNormThreads), 0, stream, p,
                       plan.norm_row_blocks);
    hipLaunchKernelGGL(match_finish_kernel, dim3(plan.finish_grid_x, plan.finish_grid_y), dim3(kAssignFinishThreads), 0, stream, p);
    return hipGetLastError();
}

}  // namespace ftk
