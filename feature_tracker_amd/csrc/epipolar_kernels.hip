// epipolar_kernels.hip — two-view outlier rejection on gfx950: RANSAC on the fundamental matrix, everything on the device.
//
//  * epipolar_scan_kernel: ONE workgroup lists the participants (status == FTK_TRACKED) in ascending index order (a block scan of
//    per-thread counts, as the track table's retire kernel, no atomic append), with their normalised coordinates and their number M.
//  * epipolar_hypothesis_kernel: one lane = one hypothesis.  The sampler is integer logic; the 8 x 9 constraint matrix lives in LDS,
//    [entry][lane], because complete pivoting indexes rows and columns at run time and a register array indexed so goes to scratch;
//    [entry][lane] makes every access of a wave one conflict-free row of 64 words.
//  * epipolar_score_kernel: a workgroup stages a tile of 256 participants in LDS and each of its waves walks the tile for 4 hypotheses,
//    whose F is wave-uniform; inliers are counted by ballot and popcount and reach memory as ONE integer atomicAdd per workgroup and
//    hypothesis.  Integer sums: no result depends on the order.
//  * epipolar_select_kernel: ONE workgroup takes the maximum of (count + 1) << 32 | ~h, denormalises the winner's F and rewrites the
//    statuses of the participants that are not its inliers.
// Every float operation below is stated in DESIGN.md 5.20 and restated in tests/epipolar_ref.c; the build has no contraction
// (-ffp-contract=off) and correctly rounded division and square root.
#include "epipolar_device.h"

namespace ftk {
namespace {

__global__ void __launch_bounds__(kEpipolarScanBlock) epipolar_scan_kernel(const EpipolarParams p) {
    __shared__ int32_t scan[kEpipolarScanBlock];
    const int tid = threadIdx.x;
    const int n = p.n;
    const int begin = min(tid * p.scan_per_thread, n), end = min(begin + p.scan_per_thread, n);
    unsigned long long mask = 0ull;
    int32_t mine = 0;
    for (int i = begin; i < end; ++i) {
        if (p.status[i] == FTK_TRACKED) {
            mask |= 1ull << (i - begin);
            ++mine;
        }
    }
    scan[tid] = mine;
    __syncthreads();
    for (int step = 1; step < kEpipolarScanBlock; step <<= 1) {  // inclusive Hillis-Steele scan
        const int32_t add = tid >= step ? scan[tid - step] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    int32_t at = scan[tid] - mine;
    for (int i = begin; i < end; ++i) {
        if ((mask >> (i - begin)) & 1ull) {
            const float2 r = reinterpret_cast<const float2 *>(p.ref_uv)[i];
            const float2 c = reinterpret_cast<const float2 *>(p.cur_uv)[i];
            p.list[at] = i;
            p.points[at] = make_float4((r.x - p.cx) * p.s, (r.y - p.cy) * p.s, (c.x - p.cx) * p.s, (c.y - p.cy) * p.s);
            ++at;
        }
    }
    if (tid == kEpipolarScanBlock - 1) {
        p.m[0] = scan[tid];
    }
}

__global__ void __launch_bounds__(kEpipolarHypBlock) epipolar_hypothesis_kernel(const EpipolarParams p) {
    __shared__ float lds[kEpipolarHypLdsFloats * kEpipolarHypBlock];
    const int lane = threadIdx.x;
    const int h = blockIdx.x * kEpipolarHypBlock + lane;
    if (h >= p.hypotheses) {
        return;  // (no barrier below)
    }
    float *const a = lds + lane;                                                             // a[(r * 9 + c) * 64]
    int *const perm = reinterpret_cast<int *>(lds + 72 * kEpipolarHypBlock) + lane;          // perm[c * 64]
    float *const fv = lds + 81 * kEpipolarHypBlock + lane;                                   // fv[c * 64]
    constexpr int L = kEpipolarHypBlock;
    const uint32_t m = (uint32_t)max(p.m[0], 0);
    // the sampler: 8 distinct positions of the participants' list
    uint32_t idx[kEpipolarSample];
    bool ok = ep_draw<kEpipolarSample>(p.seed, (uint32_t)h, m, idx);
    if (ok) {
#pragma unroll
        for (int k = 0; k < kEpipolarSample; ++k) {
            const float4 q = p.points[idx[k]];
            const float x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
            ok = ok && ep_finite(x1) && ep_finite(y1) && ep_finite(x2) && ep_finite(y2);
            a[(k * 9 + 0) * L] = x2 * x1;
            a[(k * 9 + 1) * L] = x2 * y1;
            a[(k * 9 + 2) * L] = x2;
            a[(k * 9 + 3) * L] = y2 * x1;
            a[(k * 9 + 4) * L] = y2 * y1;
            a[(k * 9 + 5) * L] = y2;
            a[(k * 9 + 6) * L] = x1;
            a[(k * 9 + 7) * L] = y1;
            a[(k * 9 + 8) * L] = 1.0f;
        }
    }
    // Gaussian elimination with complete pivoting, the null vector, unit norm (epipolar_device.h)
    float f[9];
    ok = ep_null_vector<L>(a, perm, fv, ok, f);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        p.models[(size_t)h * 9 + i] = ok ? f[i] : 0.0f;
    }
    p.valid[h] = ok ? 1 : 0;
    p.counts[h] = ok ? 0 : -1;
}

__global__ void __launch_bounds__(kEpipolarScoreTile) epipolar_score_kernel(const EpipolarParams p) {
    __shared__ float4 tile[kEpipolarScoreTile];
    const int m = min(p.m[0], p.n);
    const int base = blockIdx.x * kEpipolarScoreTile;
    if (m < kEpipolarSample || base >= m) {
        return;  // the whole workgroup: the grid covers n
    }
    const int tid = threadIdx.x;
    tile[tid] = base + tid < m ? p.points[base + tid] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    constexpr int kPerWave = kEpipolarScoreGroup / (kEpipolarScoreTile / 64);
    for (int i = 0; i < kPerWave; ++i) {
        const int h = __builtin_amdgcn_readfirstlane((int)blockIdx.y * kEpipolarScoreGroup + wave * kPerWave + i);
        if (h >= p.hypotheses) {
            break;
        }
        if (!p.valid[h]) {
            continue;
        }
        float f[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            f[e] = p.models[(size_t)h * 9 + e];
        }
        int32_t count = 0;
#pragma unroll
        for (int r = 0; r < kEpipolarScoreTile / 64; ++r) {
            const int j = r * 64 + lane;
            const bool in = base + j < m && ep_inlier(f, tile[j], p.tn2);
            count += (int32_t)__popcll(__ballot(in));
        }
        if (lane == 0 && count > 0) {
            atomicAdd(&p.counts[h], count);
        }
    }
}

__global__ void __launch_bounds__(kEpipolarScanBlock) epipolar_select_kernel(const EpipolarParams p) {
    __shared__ unsigned long long red[kEpipolarScanBlock];
    const int tid = threadIdx.x;
    unsigned long long key = 0ull;
    for (int i = 0; i < p.select_per_thread; ++i) {
        const int h = tid * p.select_per_thread + i;
        if (h < p.hypotheses) {
            const unsigned long long k = ((unsigned long long)(uint32_t)(p.counts[h] + 1) << 32) | (unsigned long long)(~(uint32_t)h);
            key = k > key ? k : key;
        }
    }
    red[tid] = key;
    __syncthreads();
    for (int step = kEpipolarScanBlock / 2; step > 0; step >>= 1) {
        if (tid < step) {
            const unsigned long long other = red[tid + step];
            if (other > red[tid]) {
                red[tid] = other;
            }
        }
        __syncthreads();
    }
    key = red[0];
    const int m = min(p.m[0], p.n);
    if ((key >> 32) == 0ull) {  // no valid hypothesis (with M < 8: none was formed)
        if (tid == 0) {
            p.best[0] = -1;
            p.n_inliers[0] = m;
        }
        if (tid < 9) {
            p.F[tid] = 0.0f;
        }
        return;
    }
    const int h = (int)(~(uint32_t)(key & 0xFFFFFFFFull));
    float f[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        f[e] = p.models[(size_t)h * 9 + e];
    }
    if (tid == 0) {
        p.best[0] = h;
        p.n_inliers[0] = (int32_t)(key >> 32) - 1;
        // F in pixels = T^T F T, T = [s 0 tx; 0 s ty; 0 0 1]: G = F T, then T^T G
        const float s = p.s, tx = -(p.cx * p.s), ty = -(p.cy * p.s);
        float g[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            g[r * 3 + 0] = f[r * 3 + 0] * s;
            g[r * 3 + 1] = f[r * 3 + 1] * s;
            g[r * 3 + 2] = (f[r * 3 + 0] * tx + f[r * 3 + 1] * ty) + f[r * 3 + 2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p.F[0 + c] = s * g[0 + c];
            p.F[3 + c] = s * g[3 + c];
            p.F[6 + c] = (tx * g[0 + c] + ty * g[3 + c]) + g[6 + c];
        }
    }
    for (int j = tid; j < m; j += kEpipolarScanBlock) {
        if (!ep_inlier(f, p.points[j], p.tn2)) {
            const int32_t i = p.list[j];
            if (i >= 0 && i < p.n) {
                p.status[i] = FTK_LARGE_RESIDUAL;
            }
        }
    }
}

}  // namespace

void epipolar_launch_scan(const EpipolarParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(epipolar_scan_kernel, dim3(1), dim3(kEpipolarScanBlock), 0, stream, p);
}

void epipolar_launch_hypotheses(uint32_t hyp_blocks, const EpipolarParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(epipolar_hypothesis_kernel, dim3(hyp_blocks), dim3(kEpipolarHypBlock), 0, stream, p);
}

void epipolar_launch_score(uint32_t score_tiles, uint32_t score_groups, const EpipolarParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(epipolar_score_kernel, dim3(score_tiles, score_groups), dim3(kEpipolarScoreTile), 0, stream, p);
}

hipError_t epipolar_launch(const EpipolarPlan &plan, const EpipolarParams &p, hipStream_t stream) {
    EpipolarParams q = p;
    q.scan_per_thread = plan.scan_per_thread;
    q.select_per_thread = plan.select_per_thread;
    epipolar_launch_scan(q, stream);
    epipolar_launch_hypotheses(plan.hyp_blocks, q, stream);
    epipolar_launch_score(plan.score_tiles, plan.score_groups, q, stream);
    hipLaunchKernelGGL(epipolar_select_kernel, dim3(1), dim3(kEpipolarScanBlock), 0, stream, q);
    return hipGetLastError();
}

}  // namespace ftk
