// raft_gemm_core.h — the implicit GEMM of RAFT's separable ConvGRU (raft_gru_kernels.hip), whose kernels are thin
// wrappers that pick a geometry and an epilogue.  Device templates only.  The conv layers of the UpdateBlock and the encoders
// (raft_conv_kernels.hip) are the same algorithm under the same contract, still written out in their kernel.
//
// The GEMM: D[co][p] = bias[co] + sum_k W[co][k] in[k][p], k in torch's own weight order (channel-major, c over the concatenation of
// the input's segments), as a chain of v_mfma_f32_32x32x2_f32 k-steps.  The numerical contract, stated here and nowhere else:
//   - k order.  The accumulator starts as the bias.  Step s adds k = 2 s (lanes 0-31), then k = 2 s + 1 (lanes 32-63), s ascending
//     over the chunks in order: one rounding per product, bit for bit the fmaf chain over ascending k.
//   - the two zeros.  A tap outside the image, and a channel beyond the input's, is a staged +0 that is multiplied like any other value
//     (torch's zero padding).  k beyond the matrix's is packed as -0 and meets a staged +0: (-0) * (+0) = -0 leaves every accumulator,
//     a -0 included, as it is.
//   - the epilogues' roundings, each one correctly rounded operation, in the order the epilogue functors state.
// The pixel is the lane-fast dimension (B operand and D column = lane & 31), the output channel the A operand's row.  The weights are
// packed so that the A operand of (row tile, k-step) is 64 consecutive floats: [m_tiles][k_steps][64], lane = 32 (k % 2) + row % 32.
//
// A workgroup of kGemmWaves waves, wm x wn (raft_gemm_plan.h), owns wm row tiles and wn tiles of 32 pixels.  Per chunk of G::kChunk
// input channels it stages the strip with its halo in LDS once, and every tap reads it at a shifted address: lanes 0-31 read 32
// consecutive floats, conflict-free.  The next chunk's strip and A operands are loaded into registers while this chunk's MFMAs run.
// An idle wave (m_tile >= m_tiles) still stages and meets every barrier.  Every index is 64-bit; no address depends on the data.
//
// A geometry G says where things lie:
//   kChunk, kSteps, kLdsFloats       input channels and k-steps of a chunk; floats of the static LDS array
//   kWpc, kCpw, kIters               waves of one strip, strips of one wave, staged positions of a lane: position lane + 64 (sub + kWpc it)
//   pitch(wn), kMaxPitch             LDS floats of a staged channel, and at wn = kGemmWaves
//   origin(tx, ty, wn, x0, y0)       the first output pixel of workgroup (tx, ty)
//   source(pos, x0, y0, yy, xx)      the input pixel staged at position pos of a strip
//   offset(k, pitch)                 constexpr: the LDS offset at which k-index k of a chunk is read
//   lane_base(wni, j)                the LDS float of pixel j of wave column wni at offset 0
//   pixel(wni, j, x0, y0, py, px)    the output pixel of (wni, j)
//   kCopyAlways                      speed only, never the result: whether a_cur = a_nxt is copied after every chunk (true) or only when
//                                    another chunk follows and the wave is active.  The GRU is 0.4 % slower at 55 x 128 without it
//                                    (DESIGN.md 6.8), so its geometries say true.
// and an epilogue is called as epi(co, b, pix, acc value) for every output channel co < out_channels of every pixel inside out_h x out_w.
// P is a parameter struct with seg[], n_seg, weights, bias, in_channels, H and W (ftk_device.h); every entry of seg[] is walked.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ftk_device.h"
#include "raft_gemm_plan.h"

namespace ftk {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kGemmThreads = 64 * kGemmWaves;

// accumulator register r of lane half kh holds this output channel (the MFMA's D layout)
__device__ __forceinline__ int gemm_out_channel(int m_tile, int r, int kh) { return m_tile * kGemmTile + (r & 3) + 8 * (r >> 2) + 4 * kh; }

template <typename G, typename P, typename Epilogue>
__device__ __forceinline__ void gemm_core(const G &geo, const P &prm, int out_channels, int out_h, int out_w, int wm, int tiles_x, int tiles_y, int chunks,
                                          int m_tiles, const Epilogue &epi) {
    constexpr int CC = G::kChunk, STEPS = G::kSteps, WPC = G::kWpc, CPW = G::kCpw, ITERS = G::kIters;
    constexpr int SEGS = sizeof(P::seg) / sizeof(ChannelSegment);
    static_assert(WPC * CC == kGemmWaves * CPW, "a chunk splits over the waves");
    static_assert(G::kLdsFloats >= CC * G::kMaxPitch, "the static LDS array holds the widest strip");
    static_assert(64 * WPC * ITERS >= G::kMaxPitch, "the staged positions cover the widest strip");
    __shared__ float s_in[G::kLdsFloats];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = kGemmWaves / wm;
    const int wmi = wave % wm, wni = wave / wm;
    const int H = prm.H, W = prm.W, Cin = prm.in_channels;
    const int64_t HW = (int64_t)H * W;
    // blockIdx.x = tx + tiles_x * (ty + tiles_y * b)
    int64_t g = blockIdx.x;
    const int tx = (int)(g % tiles_x);
    g /= tiles_x;
    const int ty = (int)(g % tiles_y);
    const int64_t b = g / tiles_y;
    int64_t x0, y0;
    geo.origin(tx, ty, wn, x0, y0);
    const int pitch = geo.pitch(wn);
    const int m_tile = blockIdx.y * wm + wmi;
    const bool active = m_tile < m_tiles;  // wave-uniform
    const int j = lane & 31, kh = lane >> 5;

    // this wave's strips are those of channels sch + 4 i of the chunk, its positions in a strip lane + 64 (sub + WPC it)
    const int sch = CC < kGemmWaves ? wave % CC : wave;
    const int sub = CC < kGemmWaves ? wave / CC : 0;
    // where this lane's staged positions lie in a channel plane (-1: outside the image or the strip: +0)
    int64_t soff[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int pos = lane + 64 * (sub + WPC * it);
        int64_t yy, xx;
        geo.source(pos, x0, y0, yy, xx);
        soff[it] = (pos < pitch && yy >= 0 && yy < H && xx >= 0 && xx < W) ? yy * W + xx : -1;
    }
    float st[CPW][ITERS];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            int c = chunk * CC + sch + kGemmWaves * i;
            const float *plane = nullptr;
#pragma unroll
            for (int s = 0; s < SEGS; ++s) {
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
                    s_in[(sch + kGemmWaves * i) * pitch + pos] = st[i][it];
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

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = gemm_out_channel(m_tile, r, kh);
        acc[r] = (active && co < out_channels) ? prm.bias[co] : 0.0f;
    }
    const int lane_base = geo.lane_base(wni, j);

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
                // this lane's k of the step within the chunk is 2 s + kh
                const int off0 = G::offset(2 * s, pitch), off1 = G::offset(2 * s + 1, pitch);
                const float bv = s_in[lane_base + (kh ? off1 : off0)];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[s], bv, acc, 0, 0, 0);
            }
        }
        __syncthreads();
        if (G::kCopyAlways || (more && active)) {
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                a_cur[s] = a_nxt[s];
            }
        }
    }

    int64_t py, px;
    geo.pixel(wni, j, x0, y0, py, px);
    if (!active || py >= out_h || px >= out_w) {
        return;
    }
    const int64_t pix = py * out_w + px;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = gemm_out_channel(m_tile, r, kh);
        if (co < out_channels) {
            epi(co, b, pix, acc[r]);
        }
    }
}

}  // namespace ftk
