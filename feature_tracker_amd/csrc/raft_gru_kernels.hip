// raft_gru_kernels.hip — RAFT's separable ConvGRU (SepConvGru.forward, src/nn_optical_flow_tracker/raft/gru.py:59-76) on gfx950:
// per pass (horizontal 1 x ks, then vertical ks x 1) two kernels, each an implicit GEMM on the f32-input matrix cores
// (v_mfma_f32_32x32x2_f32) with the activation and the element-wise tail in its epilogue:
//   gates      [z | r] = sigmoid_c(W_zr * in + b_zr) over in = x parts | h; writes z and r * h;
//   candidate  q = tanh_c(W_q * in + b_q) over in = x parts | r * h; reads z and h, writes h' = (1 - z) h + z q.
// No concatenation exists in memory: the input is a by-value list of {pointer, channels} segments read in place.
//
// The GEMM: D[co][p] = bias[co] + sum_k W[co][k] in[k][p], k = c * ks + t (channel-major, torch's own weight order), as a chain of
// MFMA k-steps in ascending order: step s adds k = 2 s (lanes 0-31) and then k = 2 s + 1 (lanes 32-63), one rounding per product,
// which is bit for bit the contract's fmaf chain.  The pixel is the lane-fast dimension (B operand and D column = lane & 31), the
// output channel the A operand's row.  The weights are packed so that the A operand of (row tile, k-step) is 64 consecutive floats;
// k beyond ks * C_in is packed as -0 and meets a staged +0: (-0) * (+0) = -0 leaves every accumulator as it is.
//
// A workgroup of 4 waves, wm x wn (sep_conv_gru_plan.h), owns wm row tiles and wn pixel tiles: 32 wn pixels of one row (horizontal) or
// wn rows of 32 pixels (vertical).  Per chunk of kGruChunk input channels it stages the strip with its halo of ks / 2 along the pass
// direction in LDS once (+0 outside the image: torch's zero padding), and every tap reads it at a shifted address: lanes 0-31 read 32
// consecutive floats, conflict-free.  The next chunk's strip and A operands are loaded into registers while this chunk's MFMAs run.
// Every index is 64-bit; no address depends on the data.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ftk_device.h"
#include "raft_math.h"
#include "sep_conv_gru_plan.h"

namespace ftk {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 64 * kGruWaves;
constexpr int kStageIters = 4;                           // 64 lanes x 4 cover the widest pitch (256)
constexpr int kStageChannels = kGruChunk / kGruWaves;    // channels of a chunk each wave stages
static_assert(kGruChunk % 2 == 0 && kGruChunk % kGruWaves == 0, "a chunk is whole k-steps and splits over the waves");
static_assert(kGruLdsFloats >= kGruChunk * 64 * kStageIters, "the static LDS array holds the widest strip");

template <int KS, bool VERT, bool GATES>
__global__ __launch_bounds__(kThreads) void sep_conv_gru_kernel(SepConvGruParams prm, int wm, int tiles_x, int tiles_y, int chunks, int m_tiles) {
    constexpr int PAD = KS / 2;
    constexpr int STEPS = kGruChunk * KS / 2;  // k-steps of a chunk
    constexpr int TAP = VERT ? kGruTile : 1;   // LDS floats between two taps
    __shared__ float s_in[kGruLdsFloats];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = kGruWaves / wm;
    const int wmi = wave % wm, wni = wave / wm;
    const int H = prm.H, W = prm.W, Ch = prm.h_channels, Cin = prm.in_channels;
    const int64_t HW = (int64_t)H * W;
    // blockIdx.x = tx + tiles_x * (ty + tiles_y * b)
    int64_t g = blockIdx.x;
    const int tx = (int)(g % tiles_x);
    g /= tiles_x;
    const int ty = (int)(g % tiles_y);
    const int64_t b = g / tiles_y;
    const int64_t x0 = VERT ? (int64_t)tx * kGruTile : (int64_t)tx * kGruTile * wn;
    const int64_t y0 = VERT ? (int64_t)ty * wn : ty;
    const int pitch = VERT ? (wn + 2 * PAD) * kGruTile : kGruTile * wn + 2 * PAD;
    const int m_tile = blockIdx.y * wm + wmi;
    const bool active = m_tile < m_tiles;  // wave-uniform; an idle wave still stages and meets every barrier
    const int j = lane & 31, kh = lane >> 5;

    // where this lane's staged positions lie in a channel plane (-1: outside the image or the strip: +0)
    int64_t soff[kStageIters];
    for (int it = 0; it < kStageIters; ++it) {
        const int pos = lane + 64 * it;
        const int64_t yy = VERT ? y0 - PAD + (pos >> 5) : y0;
        const int64_t xx = VERT ? x0 + (pos & 31) : x0 - PAD + pos;
        soff[it] = (pos < pitch && yy >= 0 && yy < H && xx >= 0 && xx < W) ? yy * W + xx : -1;
    }
    float st[kStageChannels][kStageIters];
    auto fetch = [&](int chunk) {
        for (int i = 0; i < kStageChannels; ++i) {
            int c = chunk * kGruChunk + wave + kGruWaves * i;
            const float *plane = nullptr;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (s < prm.n_seg && plane == nullptr && c < Cin) {
                    if (c < prm.seg[s].channels) {
                        plane = prm.seg[s].data + (b * prm.seg[s].channels + c) * HW;
                    } else {
                        c -= prm.seg[s].channels;
                    }
                }
            }
            for (int it = 0; it < kStageIters; ++it) {
                st[i][it] = (plane != nullptr && soff[it] >= 0) ? plane[soff[it]] : 0.0f;
            }
        }
    };
    auto stage = [&]() {
        for (int i = 0; i < kStageChannels; ++i) {
            for (int it = 0; it < kStageIters; ++it) {
                const int pos = lane + 64 * it;
                if (pos < pitch) {
                    s_in[(wave + kGruWaves * i) * pitch + pos] = st[i][it];
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

    // accumulator register r holds output channel 32 m_tile + (r & 3) + 8 (r >> 2) + 4 kh at pixel j of this wave's pixel tile
    const int out_channels = GATES ? 2 * Ch : Ch;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = m_tile * kGruTile + (r & 3) + 8 * (r >> 2) + 4 * kh;
        acc[r] = (active && co < out_channels) ? prm.bias[co] : 0.0f;
    }
    const int lane_base = wni * kGruTile + j;

    fetch(0);
    if (active) {
        load_a(0, a_cur);
    }
    for (int chunk = 0; chunk < chunks; ++chunk) {
        stage();
        __syncthreads();
        if (chunk + 1 < chunks) {
            fetch(chunk + 1);
            if (active) {
                load_a(chunk + 1, a_nxt);
            }
        }
        if (active) {
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                // this lane's k of the step within the chunk: 2 s + kh = cl * KS + t
                const int off0 = ((2 * s) / KS) * pitch + ((2 * s) % KS) * TAP;
                const int off1 = ((2 * s + 1) / KS) * pitch + ((2 * s + 1) % KS) * TAP;
                const float bv = s_in[lane_base + (kh ? off1 : off0)];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[s], bv, acc, 0, 0, 0);
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            a_cur[s] = a_nxt[s];
        }
    }

    // epilogue
    const int64_t py = VERT ? y0 + wni : y0;
    const int64_t px = VERT ? x0 + j : x0 + (int64_t)wni * kGruTile + j;
    if (!active || py >= H || px >= W) {
        return;
    }
    const int64_t pix = py * W + px;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = m_tile * kGruTile + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (co >= out_channels) {
            continue;
        }
        if (GATES) {
            const float v = sigmoid_c(acc[r]);
            if (co < Ch) {
                prm.z[(b * Ch + co) * HW + pix] = v;
            } else {
                const int64_t o = (b * Ch + (co - Ch)) * HW + pix;
                prm.rh[o] = __fmul_rn(v, prm.h[o]);
            }
        } else {
            const int64_t o = (b * Ch + co) * HW + pix;
            const float q = tanh_c(acc[r]);
            const float z = prm.z[o], hv = prm.h[o];
            const float a = __fsub_rn(1.0f, z);
            const float u = __fmul_rn(a, hv);
            const float v = __fmul_rn(z, q);
            prm.out[o] = __fadd_rn(u, v);
        }
    }
}

template <int KS, bool VERT, bool GATES>
hipError_t launch(const SepConvGruPlan &plan, const SepConvGruParams &p, hipStream_t stream) {
    hipLaunchKernelGGL((sep_conv_gru_kernel<KS, VERT, GATES>), plan.grid, plan.block, 0, stream, p, plan.wm, plan.tiles_x, plan.tiles_y, plan.chunks,
                       plan.m_tiles);
    return hipGetLastError();
}

template <int KS>
hipError_t launch_ks(const SepConvGruPlan &plan, const SepConvGruParams &p, int vertical, int gates, hipStream_t stream) {
    if (vertical) {
        return gates ? launch<KS, true, true>(plan, p, stream) : launch<KS, true, false>(plan, p, stream);
    }
    return gates ? launch<KS, false, true>(plan, p, stream) : launch<KS, false, false>(plan, p, stream);
}

}  // namespace

hipError_t sep_conv_gru_launch(const SepConvGruPlan &plan, const SepConvGruParams &p, int kernel_size, int vertical, int gates, hipStream_t stream) {
    if (plan.refused != GruRefusal::None || plan.block.x != (unsigned)kThreads || (size_t)kGruChunk * plan.pitch > (size_t)kGruLdsFloats) {
        return hipErrorInvalidValue;
    }
    return kernel_size == 5 ? launch_ks<5>(plan, p, vertical, gates, stream) : launch_ks<3>(plan, p, vertical, gates, stream);
}

}  // namespace ftk
