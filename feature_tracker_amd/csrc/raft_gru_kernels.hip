// raft_gru_kernels.hip — RAFT's separable ConvGRU (SepConvGru.forward, src/nn_optical_flow_tracker/raft/gru.py:59-76) on gfx950:
// per pass (horizontal 1 x ks, then vertical ks x 1) two kernels, each raft_gemm_core.h's implicit GEMM with the activation and the
// element-wise tail in its epilogue:
//   gates      [z | r] = sigmoid_c(W_zr * in + b_zr) over in = x parts | h; writes z and r * h;
//   candidate  q = tanh_c(W_q * in + b_q) over in = x parts | r * h; reads z and h, writes h' = (1 - z) h + z q.
// k = c * ks + t.  A workgroup owns 32 wn pixels of one row (horizontal) or wn rows of 32 pixels (vertical) and stages kGruChunk
// channels of that strip with its halo of ks / 2 along the pass direction.
#include "raft_gemm_core.h"
#include "raft_math.h"
#include "sep_conv_gru_plan.h"

namespace ftk {
namespace {

template <int KS, bool VERT>
struct GruGeometry {
    static constexpr int PAD = KS / 2;
    static constexpr int TAP = VERT ? kGemmTile : 1;  // LDS floats between two taps
    static constexpr int kChunk = kGruChunk, kSteps = kGruChunk * KS / 2, kLdsFloats = kGruLdsFloats;
    static constexpr int kWpc = 1, kCpw = kGruChunk / kGemmWaves, kIters = 4;  // 64 lanes x 4 cover the widest pitch (256)
    static constexpr bool kCopyAlways = true;
    static constexpr int kMaxPitch = VERT ? (kGemmWaves + 2 * PAD) * kGemmTile : kGemmTile * kGemmWaves + 2 * PAD;
    static_assert(kGruChunk % 2 == 0, "a chunk is whole k-steps");
    __device__ int pitch(int wn) const { return VERT ? (wn + 2 * PAD) * kGemmTile : kGemmTile * wn + 2 * PAD; }
    __device__ void origin(int tx, int ty, int wn, int64_t &x0, int64_t &y0) const {
        x0 = VERT ? (int64_t)tx * kGemmTile : (int64_t)tx * kGemmTile * wn;
        y0 = VERT ? (int64_t)ty * wn : ty;
    }
    __device__ void source(int pos, int64_t x0, int64_t y0, int64_t &yy, int64_t &xx) const {
        yy = VERT ? y0 - PAD + (pos >> 5) : y0;
        xx = VERT ? x0 + (pos & 31) : x0 - PAD + pos;
    }
    static constexpr int offset(int k, int pitch) { return (k / KS) * pitch + (k % KS) * TAP; }  // k = cl * KS + t
    __device__ int lane_base(int wni, int j) const { return wni * kGemmTile + j; }
    __device__ void pixel(int wni, int j, int64_t x0, int64_t y0, int64_t &py, int64_t &px) const {
        py = VERT ? y0 + wni : y0;
        px = VERT ? x0 + j : x0 + (int64_t)wni * kGemmTile + j;
    }
};

// z = sigmoid_c(acc) for the first h_channels rows; r = sigmoid_c(acc), then r * h (one rounded multiply) for the rest
struct GatesEpilogue {
    const float *h;
    float *z, *rh;
    int Ch;
    int64_t HW;
    __device__ void operator()(int co, int64_t b, int64_t pix, float acc) const {
        const float v = sigmoid_c(acc);
        if (co < Ch) {
            z[(b * Ch + co) * HW + pix] = v;
        } else {
            const int64_t o = (b * Ch + (co - Ch)) * HW + pix;
            rh[o] = __fmul_rn(v, h[o]);
        }
    }
};

// q = tanh_c(acc); h' = (1 - z) * h + z * q as four rounded operations in this order: 1 - z, (1 - z) * h, z * q, their sum
struct BlendEpilogue {
    const float *h, *z;
    float *out;
    int Ch;
    int64_t HW;
    __device__ void operator()(int co, int64_t b, int64_t pix, float acc) const {
        const int64_t o = (b * Ch + co) * HW + pix;
        const float q = tanh_c(acc);
        const float zv = z[o], hv = h[o];
        const float a = __fsub_rn(1.0f, zv);
        const float u = __fmul_rn(a, hv);
        const float v = __fmul_rn(zv, q);
        out[o] = __fadd_rn(u, v);
    }
};

template <int KS, bool VERT, bool GATES>
__global__ __launch_bounds__(kGemmThreads) void sep_conv_gru_kernel(SepConvGruParams prm, int wm, int tiles_x, int tiles_y, int chunks, int m_tiles) {
    const int Ch = prm.h_channels;
    const int64_t HW = (int64_t)prm.H * prm.W;
    if constexpr (GATES) {
        gemm_core(GruGeometry<KS, VERT>{}, prm, 2 * Ch, prm.H, prm.W, wm, tiles_x, tiles_y, chunks, m_tiles, GatesEpilogue{prm.h, prm.z, prm.rh, Ch, HW});
    } else {
        gemm_core(GruGeometry<KS, VERT>{}, prm, Ch, prm.H, prm.W, wm, tiles_x, tiles_y, chunks, m_tiles, BlendEpilogue{prm.h, prm.z, prm.out, Ch, HW});
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
    if (plan.refused != GruRefusal::None || plan.block.x != (unsigned)kGemmThreads || (size_t)kGruChunk * plan.pitch > (size_t)kGruLdsFloats) {
        return hipErrorInvalidValue;
    }
    return kernel_size == 5 ? launch_ks<5>(plan, p, vertical, gates, stream) : launch_ks<3>(plan, p, vertical, gates, stream);
}

}  // namespace ftk
