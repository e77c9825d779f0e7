// raft_conv_kernels.hip — the stock layers of RAFT's UpdateBlock (src/nn_optical_flow_tracker/raft/update_block.py:4-67: the motion
// encoder's five convolutions, the flow head's two, the mask head's two) on gfx950: one kernel family, conv2d_kernel<KS, RELU> for
// KS in {1, 3, 7}, stride 1, zero padding KS / 2: an implicit GEMM on the f32-input matrix cores (v_mfma_f32_32x32x2_f32) with the
// bias in the accumulators and ReLU and an output scale in the epilogue.  It is the algorithm of raft_gemm_core.h, which
// states the numerical contract, written out in the kernel: with this body behind a device function the compiler's prologue changes and
// the 256 -> 192 3 x 3 layer measured 2 % slower, so it stays here until that is solved.
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
//
// RAFT's encoders (encoder.py:4-68) add three things, all behind template parameters that default to the above, so the
// UpdateBlock's six instantiations are the code they were: a stride S of 2 for KS 1 and 3, and, with EX, a residual added to the
// accumulator before the ReLU (v = acc + res[co][y][x], one rounded add) and model.py:70-71's normalisation n = 2 (x / 255) - 1 of the
// in-image values as they are fetched (the padding stays +0), both switched by the launch's arguments.
// Stride 2: the workgroup owns 32 x wn OUTPUT pixels; output pixel (y, x) reads input (2 y + ty - PAD, 2 x + tx - PAD).  Lanes 0-31 of a
// tap would read every second float of a linear row: ds_read_b32 serves a 32-lane half from banks (address / 4) % 32, so floats 2 j and
// 2 j + 32 of lanes j and j + 16 would meet in one bank, a 2-way conflict on every B operand.  So a staged row holds its even columns
// in one plane of 32 + PAD floats and its odd columns in a second plane behind it (raft_conv_plan.h): staged column sc = 2 j + tx is
// float j + tx / 2 of plane tx % 2, lane j's bank is (base + j) % 32, 32 different banks.  Lanes 32-63 hold another tap and are
// another half.  The strip of KS 3 is 2 (wn - 1) + 3 rows of 2 x 33 floats per channel (the 66th input column is never read); KS 1
// reads even rows and columns only and stages just those, wn rows of 32.
//
// SuperPoint's VGG adds, behind POOL (default off: the instantiations above are the code they were), a 2 x 2 max-pool in
// the epilogue of stride 1, KS 1 and 3: the output is [B][Cout][H / 2][W / 2] (floored: a last odd row or column is computed and dropped),
// v = relu(acc) as above, pick(m, x) = (x > m || x != x) ? x : m, out = pick(pick(v00, v01), pick(v10, v11)); no out_scale.  x0 is a
// multiple of 32, so a horizontal pair is lanes j, j ^ 1 of one wave (one cross-lane move per accumulator); the plan of this form makes
// wn even (raft_conv_plan.h), so y0 is even and a vertical pair is waves wni, wni ^ 1 of one wmi: the wave of the odd row hands its 16
// horizontally reduced accumulators of its even lanes to the wave of the even row through s_in, free after the loop's last barrier
// (2 pairs x 16 x 32 floats), whose even lanes store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ftk_device.h"
#include "raft_conv_plan.h"

namespace ftk {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 64 * kGemmWaves;

inline __device__ const ConvParams &conv_base(const ConvParams &p) { return p; }
inline __device__ const ConvParams &conv_base(const ConvStridedParams &p) { return p.base; }

// torch's max-pool scan step: a NaN wins, and among equals (+-0 included) the one met first stays
inline __device__ float pool_pick(float m, float x) { return (x > m || x != x) ? x : m; }

template <int KS, bool RELU, int S = 1, bool EX = false, typename P = ConvParams, bool POOL = false>
__global__ __launch_bounds__(kThreads) void conv2d_kernel(P launch, int wm, int tiles_x, int tiles_y, int chunks, int m_tiles) {
    static_assert(S == 1 || (S == 2 && KS != 7), "stride 2 is built for kernel sizes 1 and 3");
    static_assert(EX || S == 1, "the strided forms take the extended parameters");
    static_assert(!POOL || (S == 1 && !EX && KS != 7), "the pooled form is stride 1, kernel sizes 1 and 3, plain parameters");
    const ConvParams &prm = conv_base(launch);
    constexpr int PAD = KS / 2;
    constexpr int CC = conv_chunk(KS);     // input channels of a chunk
    constexpr int STEPS = conv_steps(KS);  // k-steps of a chunk
    constexpr int ROW = S == 1 ? conv_row(KS) : conv_s2_row(KS);  // LDS floats of a staged row
    constexpr int PLANE = conv_s2_plane(KS);                      // stride 2: floats of the even and of the odd plane of a row
    constexpr int PITCH_MAX = S == 1 ? conv_pitch(KS, kGemmWaves) : conv_s2_pitch(KS, kGemmWaves);
    // Staging: a chunk of at least 4 channels gives each wave CC / 4 whole strips; a smaller one (KS 7: 2) gives each strip to 4 / CC waves.
    constexpr int WPC = CC < kGemmWaves ? kGemmWaves / CC : 1;  // waves of one strip
    constexpr int CPW = CC < kGemmWaves ? 1 : CC / kGemmWaves;  // strips of one wave
    constexpr int ITERS = (PITCH_MAX + 64 * WPC - 1) / (64 * WPC);
    static_assert(2 * STEPS == CC * KS * KS, "a chunk is whole k-steps");
    static_assert(CC % kGemmWaves == 0 || kGemmWaves % CC == 0, "a chunk splits over the waves");
    __shared__ float s_in[CC * PITCH_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = kGemmWaves / wm;
    const int wmi = wave % wm, wni = wave / wm;
    const int H = prm.H, W = prm.W, Cin = prm.in_channels, Cout = prm.out_channels;
    const int64_t HW = (int64_t)H * W;
    // the output's sizes: the input's at stride 1
    int OH = H, OW = W;
    if constexpr (EX) {
        OH = launch.OH, OW = launch.OW;
    }
    const int64_t OHW = (int64_t)OH * OW;
    // blockIdx.x = tx + tiles_x * (ty + tiles_y * b)
    int64_t g = blockIdx.x;
    const int tx = (int)(g % tiles_x);
    g /= tiles_x;
    const int ty = (int)(g % tiles_y);
    const int64_t b = g / tiles_y;
    const int64_t x0 = (int64_t)tx * kGemmTile;
    const int64_t y0 = (int64_t)ty * wn;
    const int pitch = (S == 1 ? wn + 2 * PAD : conv_s2_rows(KS, wn)) * ROW;
    const int m_tile = blockIdx.y * wm + wmi;
    const bool active = m_tile < m_tiles;  // wave-uniform; an idle wave still stages and meets every barrier
    const int j = lane & 31, kh = lane >> 5;

    // this wave's strips are those of channels sch + 4 i of the chunk, its positions in a strip lane + 64 (sub + WPC it)
    const int sch = CC < kGemmWaves ? wave % CC : wave;
    const int sub = CC < kGemmWaves ? wave / CC : 0;
    // where this lane's staged positions lie in a channel plane (-1: outside the image or the strip: +0)
    int64_t soff[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int pos = lane + 64 * (sub + WPC * it);
        int64_t yy = y0 - PAD + pos / ROW;
        int64_t xx = x0 - PAD + pos % ROW;
        if constexpr (S == 2) {  // row r of a 3 x 3 strip is input row 2 y0 - 1 + r, of a 1 x 1 strip 2 (y0 + r); column: 2 (float of its plane) + plane
            yy = KS == 1 ? 2 * (y0 + pos / ROW) : 2 * y0 - PAD + pos / ROW;
            xx = 2 * x0 - PAD + 2 * ((pos % ROW) % PLANE) + (pos % ROW) / PLANE;
        }
        soff[it] = (pos < pitch && yy >= 0 && yy < H && xx >= 0 && xx < W) ? yy * W + xx : -1;
    }
    float st[CPW][ITERS];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            int c = chunk * CC + sch + kGemmWaves * i;
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
                if constexpr (EX) {
                    if (launch.normalise && plane != nullptr && soff[it] >= 0) {  // model.py:70-71, one rounding per operation; the padding stays +0
                        st[i][it] = __fsub_rn(__fmul_rn(2.0f, __fdiv_rn(st[i][it], 255.0f)), 1.0f);
                    }
                }
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

    // accumulator register r holds output channel 32 m_tile + (r & 3) + 8 (r >> 2) + 4 kh at pixel j of this wave's row
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = m_tile * kGemmTile + (r & 3) + 8 * (r >> 2) + 4 * kh;
        acc[r] = (active && co < Cout) ? prm.bias[co] : 0.0f;
    }
    const int lane_base = ((S == 2 && KS > 1) ? 2 * wni : wni) * ROW + j;

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
                const int tx0 = (2 * s) % KS, tx1 = (2 * s + 1) % KS;      // stride 2: float tx / 2 of plane tx % 2
                const int off0 = ((2 * s) / KK) * pitch + (((2 * s) / KS) % KS) * ROW + (S == 1 ? tx0 : (tx0 & 1) * PLANE + tx0 / 2);
                const int off1 = ((2 * s + 1) / KK) * pitch + (((2 * s + 1) / KS) % KS) * ROW + (S == 1 ? tx1 : (tx1 & 1) * PLANE + tx1 / 2);
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

    if constexpr (POOL) {
        // the pooled epilogue: every wave meets the barrier; lanes j, j ^ 1 are columns 2 ox, 2 ox + 1, waves wni, wni ^ 1 rows 2 oy, 2 oy + 1
        constexpr int kHandOff = 16 * 32;  // floats one odd-row wave hands on: 16 accumulators of its 32 even lanes (j even, both kh)
        static_assert(2 * kHandOff <= CC * PITCH_MAX, "the hand-off of both row pairs fits the staging array");
        const int slot = (wmi + wm * (wni >> 1)) * kHandOff + kh * 16 + (j >> 1);
        float hv[16];
        if (active) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[r];
                if (RELU) {
                    v = (v < 0.0f) ? 0.0f : v;
                }
                hv[r] = pool_pick(v, __shfl_xor(v, 1));  // an even lane: pick(v(y, 2 ox), v(y, 2 ox + 1)); an odd lane's is not used
            }
            if ((wni & 1) && !(j & 1)) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s_in[slot + 32 * r] = hv[r];
                }
            }
        }
        __syncthreads();
        const int PH = H >> 1, PW = W >> 1;
        const int64_t oy = (y0 + wni) >> 1, ox = (x0 + j) >> 1;
        if (!active || (wni & 1) || (j & 1) || oy >= PH || ox >= PW) {
            return;
        }
        const int64_t PHW = (int64_t)PH * PW;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = m_tile * kGemmTile + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (co < Cout) {
                prm.out[(b * Cout + co) * PHW + oy * PW + ox] = pool_pick(hv[r], s_in[slot + 32 * r]);
            }
        }
        return;
    }
    // epilogue
    const int64_t py = y0 + wni;
    const int64_t px = x0 + j;
    if (!active || py >= OH || px >= OW) {
        return;
    }
    const int64_t pix = py * OW + px;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = m_tile * kGemmTile + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (co >= Cout) {
            continue;
        }
        float v = acc[r];
        if constexpr (EX) {
            if (launch.residual != nullptr) {
                v = __fadd_rn(v, launch.residual[(b * Cout + co) * OHW + pix]);
            }
        }
        if (RELU) {
            v = (v < 0.0f) ? 0.0f : v;  // not fmaxf: a NaN stays a NaN and -0 stays -0
        }
        prm.out[(b * Cout + co) * OHW + pix] = __fmul_rn(prm.out_scale, v);
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

template <int KS>
hipError_t launch_pool(const ConvPlan &plan, const ConvParams &p, int relu, hipStream_t stream) {
    if ((size_t)plan.chunk * plan.pitch > (size_t)conv_lds_floats(KS) || plan.chunk != conv_chunk(KS)) {
        return hipErrorInvalidValue;
    }
    if (relu) {
        hipLaunchKernelGGL((conv2d_kernel<KS, true, 1, false, ConvParams, true>), plan.grid, plan.block, 0, stream, p, plan.wm, plan.tiles_x, plan.tiles_y,
                           plan.chunks, plan.m_tiles);
    } else {
        hipLaunchKernelGGL((conv2d_kernel<KS, false, 1, false, ConvParams, true>), plan.grid, plan.block, 0, stream, p, plan.wm, plan.tiles_x, plan.tiles_y,
                           plan.chunks, plan.m_tiles);
    }
    return hipGetLastError();
}

template <int KS, int S>
hipError_t launch_strided(const ConvPlan &plan, const ConvStridedParams &p, int relu, hipStream_t stream) {
    constexpr int kLds = S == 1 ? conv_lds_floats(KS) : conv_s2_lds_floats(KS);
    static_assert(kLds * sizeof(float) <= 64 * 1024, "the static LDS of a form stays inside 64 KiB");
    if ((size_t)plan.chunk * plan.pitch > (size_t)kLds || plan.chunk != conv_chunk(KS) || plan.stride != S || p.OH != plan.out_h || p.OW != plan.out_w) {
        return hipErrorInvalidValue;
    }
    if (relu) {
        hipLaunchKernelGGL((conv2d_kernel<KS, true, S, true, ConvStridedParams>), plan.grid, plan.block, 0, stream, p, plan.wm, plan.tiles_x, plan.tiles_y,
                           plan.chunks, plan.m_tiles);
    } else {
        hipLaunchKernelGGL((conv2d_kernel<KS, false, S, true, ConvStridedParams>), plan.grid, plan.block, 0, stream, p, plan.wm, plan.tiles_x, plan.tiles_y,
                           plan.chunks, plan.m_tiles);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t raft_conv_pool_launch(const ConvPlan &plan, const ConvParams &p, int kernel_size, int relu, hipStream_t stream) {
    // the kernel pairs waves wni, wni ^ 1 and rows y0 + wni: wn must be even; the output is the plan's floored sizes
    if (plan.refused != ConvRefusal::None || plan.block.x != (unsigned)kThreads || plan.wm * plan.wn != kGemmWaves || plan.pool != 1 || plan.stride != 1 ||
        plan.wn % 2 != 0 || plan.out_h != p.H / 2 || plan.out_w != p.W / 2 || plan.out_h < 1 || plan.out_w < 1) {
        return hipErrorInvalidValue;
    }
    switch (kernel_size) {
    case 1: return launch_pool<1>(plan, p, relu, stream);
    case 3: return launch_pool<3>(plan, p, relu, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t raft_conv_strided_launch(const ConvPlan &plan, const ConvStridedParams &p, int kernel_size, int relu, hipStream_t stream) {
    if (plan.refused != ConvRefusal::None || plan.block.x != (unsigned)kThreads || plan.wm * plan.wn != kGemmWaves || plan.pool != 0) {
        return hipErrorInvalidValue;
    }
    if (plan.stride == 1 && p.residual == nullptr && !p.normalise) {
        return raft_conv_launch(plan, p.base, kernel_size, relu, stream);  // nothing of the extension is asked for: the plain forms
    }
    switch (10 * plan.stride + kernel_size) {
    case 11: return launch_strided<1, 1>(plan, p, relu, stream);
    case 13: return launch_strided<3, 1>(plan, p, relu, stream);
    case 17: return launch_strided<7, 1>(plan, p, relu, stream);
    case 21: return launch_strided<1, 2>(plan, p, relu, stream);
    case 23: return launch_strided<3, 2>(plan, p, relu, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t raft_conv_launch(const ConvPlan &plan, const ConvParams &p, int kernel_size, int relu, hipStream_t stream) {
    if (plan.refused != ConvRefusal::None || plan.block.x != (unsigned)kThreads || plan.wm * plan.wn != kGemmWaves || plan.stride != 1 || plan.pool != 0) {
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
