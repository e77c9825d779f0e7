// raft_conv_kernels.hip — the stock layers of RAFT's UpdateBlock (src/nn_optical_flow_tracker/raft/update_block.py:4-67: the motion
// encoder's five convolutions, the flow head's two, the mask head's two) on gfx950: one kernel family, conv2d_kernel<KS, RELU> for
// KS in {1, 3, 7}, stride 1, zero padding KS / 2, in the style of raft_gru_kernels.hip: an implicit GEMM on the f32-input matrix cores
// (v_mfma_f32_32x32x2_f32) with the bias in the accumulators and ReLU and an output scale in the epilogue.
// No concatenation exists in memory: the input is a by-value list of {pointer, channels} segments read in place.
//
// The GEMM: D[co][p] = bias[co] + sum_k W[co][k] in[k][p], k = (c * KS + ty) * KS + tx (torch's own weight order, c over the
// concatenation of the parts), as a chain of MFMA k-steps in ascending order: step s adds k = 2 s (lanes 0-31) and then k = 2 s + 1
// (lanes 32-63), one rounding per product, which is bit for bit the contract's fmaf chain.  The pixel is the lane-fast
// dimension (B operand and D column = lane & 31), the output channel the A operand's row.  The weights are packed so that the A operand
// of (row tile, k-step) is 64 consecutive floats; k beyond KS * KS * C_in is packed as -0 and meets a staged +0: (-0) * (+0) = -0
// leaves every accumulator as it is.  A tap outside the image is a staged +0 that is multiplied like any other value.
// Epilogue, in this order: v = (acc < 0) ? +0 : acc if RELU (a NaN and -0 pass), then out = out_scale * v (one rounded multiply).
//
// A workgroup of 4 waves, wm x wn (raft_conv_plan.h), owns wm row tiles and wn rows of 32 pixels.  Per chunk of conv_chunk(KS) input
// channels it stages the strip with its halo of KS / 2 on all four sides in LDS once, (wn + 2 PAD) rows of (32 + 2 PAD) floats per
// channel (+0 outside the image: torch's zero padding), and every tap reads it at a shifted address: lanes 0-31 read 32 consecutive
// floats, conflict-free.  The next chunk's strip and A operands are loaded into registers while this chunk's MFMAs run.
// Every index is 64-bit; no address depends on the data.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ftk_device.h"
#include "raft_conv_plan.h"

namespace ftk {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 64 * kConvWaves;

template <int KS, bool RELU>
__global__ __launch_bounds__(kThreads) void conv2d_kernel(ConvParams prm, int wm, int tiles_x, int tiles_y, int chunks, int m_tiles) {
    constexpr int PAD = KS / 2;
    constexpr int CC = conv_chunk(KS);     // input channels of a chunk
    constexpr int STEPS = conv_steps(KS);  // k-steps of a chunk
    constexpr int ROW = conv_row(KS);      // LDS floats of a staged row
    // Staging: a chunk of at least 4 channels gives each wave CC / 4 whole strips; a smaller one (KS 7: 2) gives each strip to 4 / CC waves.
    constexpr int WPC = CC < kConvWaves ? kConvWaves / CC : 1;  // waves of one strip
    constexpr int CPW = CC < kConvWaves ? 1 : CC / kConvWaves;  // strips of one wave
    constexpr int ITERS = (conv_pitch(KS, kConvWaves) + 64 * WPC - 1) / (64 * WPC);
    static_assert(2 * STEPS == CC * KS * KS, "a chunk is whole k-steps");
    static_assert(CC % kConvWaves == 0 || kConvWaves % CC == 0, "a chunk splits over the waves");
    __shared__ float s_in[conv_lds_floats(KS)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = kConvWaves / wm;
    const int wmi = wave % wm, wni = wave / wm;
    const int H = prm.H, W = prm.W, Cin = prm.in_channels, Cout = prm.out_channels;
    const int64_t HW = (int64_t)H * W;
    // blockIdx.x = tx + tiles_x * (ty + tiles_y * b)
    int64_t g = blockIdx.x;
    const int tx = (int)(g % tiles_x);
    g /= tiles_x;
    const int ty = (int)(g % tiles_y);
    const int64_t b = g / tiles_y;
    const int64_t x0 = (int64_t)tx * kConvTile;
    const int64_t y0 = (int64_t)ty * wn;
    const int pitch = (wn + 2 * PAD) * ROW;
    const int m_tile = blockIdx.y * wm + wmi;
    const bool active = m_tile < m_tiles;  // wave-uniform; an idle wave still stages and meets every barrier
    const int j = lane & 31, kh = lane >> 5;

    // this wave's strips are those of channels sch + 4 i of the chunk, its positions in a strip lane + 64 (sub + WPC it)
    const int sch = CC < kConvWaves ? wave % CC : wave;
    const int sub = CC < kConvWaves ? wave / CC : 0;
    // where this lane's staged positions lie in a channel plane (-1: outside the image or the strip: +0)
    int64_t soff[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int pos = lane + 64 * (sub + WPC * it);
        const int64_t yy = y0 - PAD + pos / ROW;
        const int64_t xx = x0 - PAD + pos % ROW;
        soff[it] = (pos < pitch && yy >= 0 && yy < H && xx >= 0 && xx < W) ? yy * W + xx : -1;
    }
    float st[CPW][ITERS];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            int c = chunk * CC + sch + kConvWaves * i;
            const float *plane = nullptr;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                if (s < prm.n_seg && plane == nullptr && c < Cin) {
                    if (c < prm.seg[s].channels) {
                        plane = prm.seg[s].data + (b * prm.seg[s].channels + c) * HW;
                    } else {
                        c -= prm.seg[s].channels;
                    }
                }
            }
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                st[i][it] = (plane != nullptr && soff[it] >= 0) ? plane[soff[it]] : 0.0f;
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                const int pos = lane + 64 * (sub + WPC * it);
                if (pos < pitch) {
                    s_in[(sch + kConvWaves * i) * pitch + pos] = st[i][it];
                }
            }
        }
    };
    const int k_steps = chunks * STEPS;
    const float *wp = prm.weights + ((int64_t)(active ? m_tile : 0) * k_steps) * 64 + lane;
    float a_cur[STEPS], a_nxt[STEPS];
    auto load_a = [&](int chunk, float (&a)[STEPS]) {
        const float *src = wp + (int64_t)chunk * STEPS * 64;
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            a[s] = src[s * 64];
        }
    };

    // accumulator register r holds output channel 32 m_tile + (r & 3) + 8 (r >> 2) + 4 kh at pixel j of this wave's row
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = m_tile * kConvTile + (r & 3) + 8 * (r >> 2) + 4 * kh;
        acc[r] = (active && co < Cout) ? prm.bias[co] : 0.0f;
    }
    const int lane_base = wni * ROW + j;

    fetch(0);
    if (active) {
        load_a(0, a_cur);
    }
    for (int chunk = 0; chunk < chunks; ++chunk) {
        stage();
        __syncthreads();
        const bool more = chunk + 1 < chunks;
        if (more) {
            fetch(chunk + 1);
            if (active) {
                load_a(chunk + 1, a_nxt);
            }
        }
        if (active) {
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                // this lane's k of the step within the chunk: 2 s + kh = (cl * KS + ty) * KS + tx
                constexpr int KK = KS * KS;
                const int off0 = ((2 * s) / KK) * pitch + (((2 * s) / KS) % KS) * ROW + (2 * s) % KS;
                const int off1 = ((2 * s + 1) / KK) * pitch + (((2 * s + 1) / KS) % KS) * ROW + (2 * s + 1) % KS;
                const float bv = s_in[lane_base + (kh ? off1 : off0)];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[s], bv, acc, 0, 0, 0);
            }
        }
        __syncthreads();
        if (more && active) {
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                a_cur[s] = a_nxt[s];
            }
        }
    }

    // epilogue
    const int64_t py = y0 + wni;
    const int64_t px = x0 + j;
    if (!active || py >= H || px >= W) {
        return;
    }
    const int64_t pix = py * W + px;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = m_tile * kConvTile + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (co >= Cout) {
            continue;
        }
        float v = acc[r];
        if (RELU) {
            v = (v < 0.0f) ? 0.0f : v;  // not fmaxf: a NaN stays a NaN and -0 stays -0
        }
        prm.out[(b * Cout + co) * HW + pix] = __fmul_rn(prm.out_scale, v);
    }
}

template <int KS>
hipError_t launch_ks(const ConvPlan &plan, const ConvParams &p, int relu, hipStream_t stream) {
    if ((size_t)plan.chunk * plan.pitch > (size_t)conv_lds_floats(KS) || plan.chunk != conv_chunk(KS)) {
        return hipErrorInvalidValue;
    }
    if (relu) {
        hipLaunchKernelGGL((conv2d_kernel<KS, true>), plan.grid, plan.block, 0, stream, p, plan.wm, plan.tiles_x, plan.tiles_y, plan.chunks, plan.m_tiles);
    } else {
        hipLaunchKernelGGL((conv2d_kernel<KS, false>), plan.grid, plan.block, 0, stream, p, plan.wm, plan.tiles_x, plan.tiles_y, plan.chunks, plan.m_tiles);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t raft_conv_launch(const ConvPlan &plan, const ConvParams &p, int kernel_size, int relu, hipStream_t stream) {
    if (plan.refused != ConvRefusal::None || plan.block.x != (unsigned)kThreads || plan.wm * plan.wn != kConvWaves) {
        return hipErrorInvalidValue;
    }
    switch (kernel_size) {
    case 1: return launch_ks<1>(plan, p, relu, stream);
    case 3: return launch_ks<3>(plan, p, relu, stream);
    case 7: return launch_ks<7>(plan, p, relu, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace ftk
