// lightglue_adaptive_kernels.hip — LightGlue's adaptive depth and width on gfx950 (LightGlue.match_adaptive): the
// per-layer steps between the transformer layers and the two steps around the assignment head, with no copy to the host.
//
//  * confidence_kernel: a thread owns one live row of either set and runs the two fmaf chains over its columns ascending, from the
//    biases: conf = sigmoid_c(token(x)), mt = sigmoid_c(matchability(x)).
//  * decide_kernel: ONE workgroup makes every decision of a layer.  The integer count u of rows with conf < t and the stop test; the
//    keep masks of both sides, whose exclusive prefix sums place the kept rows at the front in their order; the new counts; `layers`
//    of the rows that leave.  It writes, per destination row, the source row (identity when stopped or not pruning).
//  * gather_kernel: one wave per destination row moves the descriptor row, both planes of the rotary encoding and `ind` from one half
//    of a ping-pong pair into the other, so no workgroup overwrites what another still reads.
//  * head_select_kernel: the weights and bias of log_assignment.{stop_layer} out of the packed [L][D + 1][D] and [L][D + 1] into the
//    staging buffers ftk_match_assignment_device reads, and match_index = -1, status = unmatched for every original row.
//  * remap_kernel: match_index[ind0[r]] = ind1[m[r]] for the live rows, and `layers` of the rows that stayed to the end.
//
// Every float operation is written out; with -ffp-contract=off the results are bit-identical to tests/lightglue_adaptive_ref.c.
// Every index is 64-bit; an index read from memory (a count, a source row, an original index, the stop layer) is clamped to its
// array before it addresses anything.
#include "lightglue_adaptive_plan.h"
#include "mfma_tile_gemm.h"
#include "raft_math.h"

namespace ftk {
namespace {

__global__ void __launch_bounds__(kAdaptiveConfThreads) confidence_kernel(const ConfidenceParams p) {
    if (p.gate && p.gate[0] != 0) {  // workgroup-uniform
        return;
    }
    const int rows0 = p.rows0, rows = p.rows0 + p.rows1;
    const int row = blockIdx.x * kAdaptiveConfThreads + threadIdx.x;
    if (row >= rows) {
        return;
    }
    const bool first = row < rows0;
    const int local = first ? row : row - rows0;
    if (local >= (first ? valid_count(p.live0, rows0) : valid_count(p.live1, p.rows1))) {
        return;
    }
    const float *x = (first ? p.desc0 : p.desc1) + (size_t)local * p.dim;
    float zc = p.token_b[0], zm = p.match_b[0];
    for (int c = 0; c < p.dim; ++c) {
        const float v = x[c];
        zc = fmaf(v, p.token_w[c], zc);
        zm = fmaf(v, p.match_w[c], zm);
    }
    p.conf[row] = sigmoid_c(zc);
    p.mt[row] = sigmoid_c(zm);
}

// The exclusive prefix sum of one value per thread over the workgroup (Hillis-Steele in LDS); *total receives the sum.
__device__ __forceinline__ int block_exclusive_sum(int value, int *scratch, int *total) {
    const int t = threadIdx.x;
    __syncthreads();
    scratch[t] = value;
    __syncthreads();
    for (int off = 1; off < kAdaptiveDecideThreads; off <<= 1) {
        const int add = t >= off ? scratch[t - off] : 0;
        __syncthreads();
        scratch[t] += add;
        __syncthreads();
    }
    *total = scratch[kAdaptiveDecideThreads - 1];
    return scratch[t] - value;
}

__global__ void __launch_bounds__(kAdaptiveDecideThreads) decide_kernel(const AdaptStepParams p) {
    __shared__ int scratch[kAdaptiveDecideThreads];
    const int t = threadIdx.x;
    const int rows_of[2] = {p.rows0, p.rows1};
    // the state as the step found it; it is written only behind the last barrier
    const int stopped = p.state[kStateStopped];
    const int live[2] = {min(max(p.state[kStateLive0], 0), p.rows0), min(max(p.state[kStateLive1], 0), p.rows1)};
    int stop = 0;
    if (!stopped && p.depth_on) {
        int unsure = 0;
        for (int side = 0; side < 2; ++side) {
            const float *conf = p.conf + (side ? p.rows0 : 0);
            const int per = (rows_of[side] + kAdaptiveDecideThreads - 1) / kAdaptiveDecideThreads;
            const int end = min((t + 1) * per, live[side]);
            for (int r = t * per; r < end; ++r) {
                unsure += conf[r] < p.threshold ? 1 : 0;
            }
        }
        int u;
        block_exclusive_sum(unsure, scratch, &u);
        const int points = valid_count(p.count0, p.rows0) + valid_count(p.count1, p.rows1);
        stop = points > 0 && __fsub_rn(1.0f, __fdiv_rn((float)u, (float)points)) > p.depth ? 1 : 0;
    }
    const bool prune = !stopped && !stop && p.width_on;
    int kept_of[2];
    for (int side = 0; side < 2; ++side) {
        const int base = side ? p.rows0 : 0;
        const float *conf = p.conf + base, *mt = p.mt + base;
        int *src = side ? p.src1 : p.src0, *layers = side ? p.layers1 : p.layers0;
        const int *ind = side ? p.ind_in1 : p.ind_in0;
        const bool here = prune && live[side] > p.min_keypoints;
        const int per = (rows_of[side] + kAdaptiveDecideThreads - 1) / kAdaptiveDecideThreads;
        const int begin = t * per, end = min((t + 1) * per, live[side]);
        unsigned mask = 0;  // per <= 16 rows
        int kept = 0;
        for (int r = begin; r < end; ++r) {
            const bool keep = !here || mt[r] > p.width || (p.depth_on && conf[r] <= p.threshold);
            mask |= keep ? 1u << (r - begin) : 0u;
            kept += keep ? 1 : 0;
        }
        int at = block_exclusive_sum(kept, scratch, &kept_of[side]);
        for (int r = begin; r < end; ++r) {
            if (mask >> (r - begin) & 1u) {
                src[at++] = r;  // at < kept_of[side] <= live[side] <= rows
            } else {
                const int original = ind[r];
                if (original >= 0 && original < rows_of[side]) {
                    layers[original] = p.layer + 1;
                }
            }
        }
    }
    __syncthreads();
    if (t == 0 && !stopped) {
        p.state[kStateLive0] = kept_of[0];
        p.state[kStateLive1] = kept_of[1];
        if (stop) {
            p.state[kStateStopped] = 1;
            p.state[kStateStopLayer] = p.layer;
        }
    }
}

__global__ void __launch_bounds__(kAdaptiveGatherThreads) gather_kernel(const AdaptStepParams p) {
    const int lane = threadIdx.x;
    const int row = blockIdx.x;  // < rows0 + rows1: the grid is the plan's gather_blocks
    const bool first = row < p.rows0;
    const int rows = first ? p.rows0 : p.rows1, dst = first ? row : row - p.rows0;
    const int live = min(max(p.state[first ? kStateLive0 : kStateLive1], 0), rows);  // the NEW count: decide_kernel ran before
    if (dst >= live) {
        return;
    }
    const int from = min(max((first ? p.src0 : p.src1)[dst], 0), rows - 1);
    const float *din = (first ? p.desc_in0 : p.desc_in1) + (size_t)from * p.dim;
    float *dout = (first ? p.desc_out0 : p.desc_out1) + (size_t)dst * p.dim;
    for (int c = lane; c < p.dim; c += kAdaptiveGatherThreads) {
        dout[c] = din[c];
    }
    const float *ein = first ? p.enc_in0 : p.enc_in1;
    float *eout = first ? p.enc_out0 : p.enc_out1;
    const size_t plane = (size_t)rows * p.head_dim;
    for (int c = lane; c < 2 * p.head_dim; c += kAdaptiveGatherThreads) {
        const size_t pl = c < p.head_dim ? 0 : plane, e = (size_t)(c < p.head_dim ? c : c - p.head_dim);
        eout[pl + (size_t)dst * p.head_dim + e] = ein[pl + (size_t)from * p.head_dim + e];
    }
    if (lane == 0) {
        (first ? p.ind_out0 : p.ind_out1)[dst] = (first ? p.ind_in0 : p.ind_in1)[from];
    }
}

__global__ void __launch_bounds__(kAdaptiveCopyThreads) head_select_kernel(const FinishParams p) {
    const size_t d = (size_t)p.dim, w_floats = (d + 1) * d, b_floats = d + 1;
    const size_t layer = (size_t)min(max(p.state[kStateStopLayer], 0), p.n_layers - 1);
    const float *w = p.head_w + layer * w_floats, *b = p.head_b + layer * b_floats;
    const size_t total = w_floats + b_floats + (size_t)p.rows0, step = (size_t)gridDim.x * kAdaptiveCopyThreads;
    for (size_t i = (size_t)blockIdx.x * kAdaptiveCopyThreads + threadIdx.x; i < total; i += step) {
        if (i < w_floats) {
            p.sel_w[i] = w[i];
        } else if (i < w_floats + b_floats) {
            p.sel_b[i - w_floats] = b[i - w_floats];
        } else {
            p.match_index[i - w_floats - b_floats] = -1;
            p.status[i - w_floats - b_floats] = (uint8_t)kAdaptiveUnmatched;
        }
    }
}

__global__ void __launch_bounds__(kAdaptiveCopyThreads) remap_kernel(const FinishParams p) {
    const int row = blockIdx.x * kAdaptiveCopyThreads + threadIdx.x;
    if (row >= p.rows0 + p.rows1) {
        return;
    }
    const int live0 = min(max(p.state[kStateLive0], 0), p.rows0), live1 = min(max(p.state[kStateLive1], 0), p.rows1);
    const int took_part = min(max(p.state[kStateStopLayer], 0), p.n_layers - 1) + 1;
    if (row < p.rows0) {
        if (row >= live0) {
            return;
        }
        const int original = p.ind0[row];
        if (original < 0 || original >= p.rows0) {
            return;
        }
        const int m = p.match[row];
        const bool beyond = m >= live1;  // (only a row of -inf alone under min_score = -inf matches a pruned column)
        p.match_index[original] = m >= 0 && !beyond ? p.ind1[m] : -1;
        p.status[original] = beyond ? (uint8_t)kAdaptiveUnmatched : p.status_in[row];
        p.layers0[original] = took_part;
    } else {
        const int r = row - p.rows0;
        if (r >= live1) {
            return;
        }
        const int original = p.ind1[r];
        if (original >= 0 && original < p.rows1) {
            p.layers1[original] = took_part;
        }
    }
}

}  // namespace

hipError_t confidence_launch(const LightglueAdaptivePlan &plan, const ConfidenceParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(confidence_kernel, dim3(plan.conf_blocks), dim3(kAdaptiveConfThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t adapt_step_launch(const LightglueAdaptivePlan &plan, const AdaptStepParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(decide_kernel, dim3(plan.decide_blocks), dim3(kAdaptiveDecideThreads), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        return e;
    }
    hipLaunchKernelGGL(gather_kernel, dim3(plan.gather_blocks), dim3(kAdaptiveGatherThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t head_select_launch(const LightglueAdaptivePlan &plan, const FinishParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(head_select_kernel, dim3(plan.select_blocks), dim3(kAdaptiveCopyThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t remap_launch(const LightglueAdaptivePlan &plan, const FinishParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(remap_kernel, dim3(plan.remap_blocks), dim3(kAdaptiveCopyThreads), 0, stream, p);
    return hipGetLastError();
}

}  // namespace ftk
