// raft_points_kernels.hip — sparse feature tracking from RAFT's coarse flow: per feature point the bilinear sample of the
// convex-upsampled flow (Raft.UpsampleFlow, src/nn_optical_flow_tracker/raft/model.py:48-64) at the point, the tracked point, its
// TrackStatus and, with a backward flow, the forward-backward error, in ONE kernel.  No fine flow field is ever stored: a fine value is
// computed where a point reads it.
//
// A workgroup of 256 threads owns kTile = 64 consecutive points of one batch entry; lane q = tid % 4 of a point's quad of lanes takes the
// corner (q / 2, q % 2) of the point's fine cell: the 9 logits of that fine pixel (64 H W floats apart), the padded 3 x 3 neighbourhood of
// 8 * flow of its coarse pixel, and steps 1 to 6 of DESIGN.md 5.12, the very floats flow_upsample_kernel writes there.  The four corner
// values cross the quad by __shfl and every lane of the quad forms the same three fmaf; with a backward pair the quad does it all a
// second time at the tracked point.  Lane 0 of the quad stores.
// Control flow: every lane of a wave reaches every __shfl; a point that is done (or past N) only stops loading.  Addresses: a sample is
// taken only at a point that passed the inside test, 0 <= u <= image_cols - 1 <= 8 W - 1 in float32 (exact: the entry holds 8 W and 8 H
// to 2^24), so floorf(u) is an integer in 0 .. 8 W - 1 and the neighbour is clamped to 8 W - 1; NaN fails the test.  Every index is
// 64-bit.  Arithmetic: the contract's sequence of correctly rounded float32 operations (-ffp-contract=off), bit-identical to the scalar
// restatement (tests/flow_points_ref.c).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ftk_device.h"
#include "raft_math.h"

namespace ftk {
namespace {

constexpr int kTile = kFlowPointsTile;
constexpr int kThreads = 4 * kTile;
static_assert(kTile == FTK_FLOW_POINTS_TILE, "include/ftk.h states the tile");
static_assert(kThreads % 64 == 0, "whole waves, and a quad never straddles two");

struct Pair {
    float x, y;
};

// contract step 1: NaN fails
__device__ __forceinline__ bool inside(float u, float v, float last_col, float last_row) {
    return u >= 0.0f && u <= last_col && v >= 0.0f && v <= last_row;
}

// The two flow components of fine pixel (iy, ix) of batch entry b: steps 1 to 6 of DESIGN.md 5.12, as flow_upsample_kernel computes them.
__device__ __forceinline__ Pair fine_value(const float *__restrict__ flow, const float *__restrict__ mask, int64_t b, int H, int W, int iy, int ix,
                                           float mask_scale) {
    const int y = iy >> 3, i = iy & 7, x = ix >> 3, j = ix & 7;
    const int64_t HW = (int64_t)H * W;
    const float *mp = mask + (b * 576 + i * 8 + j) * HW + (int64_t)y * W + x;
    float xs[9], f0[9], f1[9];
    for (int k = 0; k < 9; ++k) {
        xs[k] = mp[(int64_t)(k * 64) * HW] * mask_scale;  // step 1
    }
    for (int k = 0; k < 9; ++k) {  // step 5
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const int64_t at = (b * 2) * HW + (int64_t)yy * W + xx;
        f0[k] = in ? 8.0f * flow[at] : 0.0f;
        f1[k] = in ? 8.0f * flow[at + HW] : 0.0f;
    }
    float m = xs[0];  // step 2
    for (int k = 1; k < 9; ++k) {
        if (xs[k] > m) {
            m = xs[k];
        }
    }
    float e[9];
    for (int k = 0; k < 9; ++k) {
        e[k] = exp_c(xs[k] - m);  // step 3
    }
    float s = e[0] + e[1];  // step 4
    for (int k = 2; k < 9; ++k) {
        s = s + e[k];
    }
    Pair a{0.0f, 0.0f};
    for (int k = 0; k < 9; ++k) {  // step 6
        const float w = e[k] / s;
        const float p0 = f0[k] * w, p1 = f1[k] * w;
        a.x = k == 0 ? p0 : a.x + p0;
        a.y = k == 0 ? p1 : a.y + p1;
    }
    return a;
}

// Contract step 2, S(flow, mask, u, v), by the quad of lanes of one point; `live` is the same in the four lanes, (u, v) is inside when it is
// set, and the result is the same in the four lanes (0 when not live).
__device__ __forceinline__ Pair sample(const float *__restrict__ flow, const float *__restrict__ mask, int64_t b, int H, int W, float u, float v,
                                       float mask_scale, bool live, int corner, int quad_base) {
    Pair mine{0.0f, 0.0f};
    float fx = 0.0f, fy = 0.0f;
    if (live) {
        const float x0 = floorf(u), y0 = floorf(v);
        fx = u - x0;
        fy = v - y0;
        const int ix0 = (int)x0, iy0 = (int)y0;
        const int ix1 = min(ix0 + 1, 8 * W - 1), iy1 = min(iy0 + 1, 8 * H - 1);
        mine = fine_value(flow, mask, b, H, W, (corner & 2) ? iy1 : iy0, (corner & 1) ? ix1 : ix0, mask_scale);
    }
    Pair c[4];  // v00, v01, v10, v11
    for (int q = 0; q < 4; ++q) {
        c[q].x = __shfl(mine.x, quad_base + q);
        c[q].y = __shfl(mine.y, quad_base + q);
    }
    Pair r;
    const float top_x = fmaf(fx, c[1].x - c[0].x, c[0].x), bot_x = fmaf(fx, c[3].x - c[2].x, c[2].x);
    r.x = fmaf(fy, bot_x - top_x, top_x);
    const float top_y = fmaf(fx, c[1].y - c[0].y, c[0].y), bot_y = fmaf(fx, c[3].y - c[2].y, c[2].y);
    r.y = fmaf(fy, bot_y - top_y, top_y);
    return r;
}

__global__ __launch_bounds__(kThreads) void flow_track_points_kernel(FlowPointsParams prm, int tiles) {
    const int tid = threadIdx.x;
    const int corner = tid & 3, quad_base = (tid & 63) & ~3;
    const int64_t b = blockIdx.x / tiles;
    const int64_t n = (int64_t)(blockIdx.x % tiles) * kTile + (tid >> 2);
    const bool present = n < prm.N;
    const int64_t at = b * prm.N + n;
    const int H = prm.H, W = prm.W;
    const float last_col = (float)(prm.image_cols - 1), last_row = (float)(prm.image_rows - 1);

    float u = 0.0f, v = 0.0f;
    if (present) {
        u = prm.points[2 * at];
        v = prm.points[2 * at + 1];
    }
    uint8_t status = FTK_OUTSIDE;  // step 1
    float cur_x = u, cur_y = v, e2 = 0.0f;
    bool live = present && inside(u, v, last_col, last_row);

    const Pair s = sample(prm.flow, prm.mask, b, H, W, u, v, prm.mask_scale, live, corner, quad_base);
    if (live) {  // step 3
        const float x = u + s.x, y = v + s.y;
        if (!(isfinite(x) && isfinite(y))) {
            status = FTK_NUMERIC_ERROR;
            live = false;
        } else {
            cur_x = x;
            cur_y = y;
            live = inside(x, y, last_col, last_row);
            status = live ? FTK_TRACKED : FTK_OUTSIDE;
        }
    }
    if (prm.flow_back) {  // step 4; the same in every lane of the grid
        const Pair sb = sample(prm.flow_back, prm.mask_back, b, H, W, cur_x, cur_y, prm.mask_scale, live, corner, quad_base);
        if (live) {
            const float ex = (cur_x + sb.x) - u, ey = (cur_y + sb.y) - v;
            e2 = fmaf(ey, ey, ex * ex);
            if (!(e2 <= prm.fb_threshold * prm.fb_threshold)) {
                status = FTK_LARGE_RESIDUAL;
            }
        }
    }
    if (present && corner == 0) {
        prm.cur_points[2 * at] = cur_x;
        prm.cur_points[2 * at + 1] = cur_y;
        prm.status[at] = status;
        if (prm.fb_error2) {
            prm.fb_error2[at] = e2;
        }
    }
}

}  // namespace

hipError_t flow_track_points_launch(const FlowPointsParams &p, hipStream_t stream) {
    const int64_t tiles = ((int64_t)p.N + kTile - 1) / kTile;
    const int64_t groups = tiles * p.B;
    if (groups < 1 || groups > 0x7fffffff) {
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(flow_track_points_kernel, dim3((unsigned)groups), dim3(kThreads), 0, stream, p, (int)tiles);
    return hipGetLastError();
}

}  // namespace ftk
