// match_plan.cpp — hamming_plan, cosine_plan and direct_plan (match_plan.h): every shape decision of the matchers' and the direct
// method's launches, in one place, from values alone.
#include "match_plan.h"

#include <algorithm>

namespace ftk {
namespace {

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
int ceil_div(long long x, long long d) { return (int)((x + d - 1) / d); }

// Direct method: a batch is spread over the chip (1 + NP workgroups per problem) while at least two producer workgroups per problem
// fit beside the others (NP = 32 for up to six problems, then what the 224 usable workgroups of a whole MI355X allow).  Round 5, same box,
// batches of 300 points x 13 x 13 x 4 levels, spread / one workgroup per problem, ms: 1 problem 1.01 / 1.81,
// 6: 1.05 / 1.85, 12: 1.11 / 1.85, 24 (NP 8): 1.16 / 1.86, 32 (6): 1.21 / 1.86, 44 (4): 1.30 / 1.87, 56 (3): 1.41 / 1.89, 64 (2): 1.39 /
// 1.89, 74 (2): 1.54 / 1.88, 100 (1): 2.03 / 1.93 — one producer workgroup does not keep up with its consumer's chain, two do
// (profiles/r5_direct_spread_consumer.txt).  Beyond that one workgroup per problem IS the fast form, and its time is one problem's.
constexpr int kDirectSpreadMaxProblems = 112;  // (two producers each no longer fit from 75 problems on a whole device: the fit decides)
constexpr int kDirectSpreadMinProducers = 2;

}  // namespace

int32_t hamming_device_words(int32_t n_words) {
    if (n_words > 16) {
        return n_words;
    }
    int32_t w = 1;
    while (w < n_words) {
        w *= 2;
    }
    return w;
}

HammingPlan hamming_plan(const HammingPlanInput &in) {
    HammingPlan pl = {};
    pl.box_grid = pl.epilogue_grid = dim3(0);
    const int32_t nw = hamming_device_words(in.n_words);
    pl.dev_words = nw;
    pl.keys_clean = in.keys_given ? 0 : 1;
    // Split the candidate range finely (a workgroup covers 512 reference descriptors — two per thread,
    // matcher_kernels.hip — and as few as 64 candidates): measured at 10 000 x 10 000, 40 / 80 / 160
    // splits take 85 / 74 / 69 us; the scan is pure VALU work and small workgroups even out the tail.
    const int row_blocks = ceil_div(in.n_ref, kMatchRowsPerBlock);
    const int splits = std::max(1, std::min(ceil_div(4096, row_blocks), ceil_div(in.n_cur, 64)));
    int per = ceil_div(ceil_div(in.n_cur, splits), 64) * 64;
    // Which scan: 256- and 512-bit descriptors go to the matrix cores (matcher_kernels.hip, hamming_match_mfma_kernel: faster at every
    // size measured, 300 x 300 to 10 000 x 10 000; it addresses the candidates with 32-bit byte offsets); other widths to the popcount
    // scan with the candidates on the scalar path.  FTK_MATCH_KERNEL=mfma|scalar forces one (experiment switch).
    const bool mfma = in.n_bits > 0 && (nw == 8 || nw == 16) && (long long)in.n_cur * nw * 4 < (1ll << 31) && (in.kernel == kPlanNotSet || in.kernel == 1);
    if (mfma) {
        // One wave per workgroup: kMfmaRows rows and one split of the candidates, in whole tiles.  Two waves fit a SIMD (registers):
        // one round of at most 2048 waves, the splits as even as the tile count allows.
        const int mfma_splits = std::max(1, 2048 / ceil_div(in.n_ref, kMfmaRows));
        per = std::min(ceil_div(ceil_div(in.n_cur, kMfmaTile), mfma_splits), kMfmaMaxTilesPerSplit) * kMfmaTile;
    }
    pl.matrix_cores = mfma ? 1 : 0;
    pl.cur_per_block = per;
    const int launched_splits = ceil_div(in.n_cur, per);
    // NearbyMatch from a few thousand candidates on: bounding boxes for the early exit of workgroups whose candidates cannot reach any
    // window of their rows (matcher_kernels.hip)
    if (in.nearby && in.n_bits > 0 && in.n_cur >= 2048) {
        pl.n_boxes = (size_t)row_blocks + (size_t)launched_splits;
    }
    // Small calls run as ONE launch with no workspace (matcher_kernels.hip hamming_match_small_kernel); FTK_MATCH_SMALL=0: never
    const bool small = in.small != 0 && nw <= 16 && in.n_bits > 0 && in.n_cur < kSmallNoIndex && (long long)in.n_cur * nw <= kSmallMatchRowWork &&
                       (long long)in.n_ref * in.n_cur * nw <= kSmallMatchWork;
    pl.scan_block = dim3(kMatchBlock);
    if (small) {
        pl.form = HammingForm::Small;
        pl.scan_grid = dim3(ceil_div(in.n_ref, kMatchBlock / kWave));  // a wave per reference row
        return pl;
    }
    if (nw > 16 || in.n_bits == 0) {
        // the generic scan; or ComputeDistance's "empty descriptor" answer (kMaxInt32), which does not fit the packed key: plain scan
        pl.form = nw > 16 ? HammingForm::Generic : HammingForm::Plain;
        pl.scan_grid = dim3(ceil_div(in.n_ref, kMatchBlock), launched_splits);
    } else if (mfma) {
        pl.form = HammingForm::MatrixCores;
        pl.scan_grid = dim3(ceil_div(in.n_ref, kMfmaRows), launched_splits);
        pl.scan_block = dim3(kWave);
    } else {
        pl.form = HammingForm::Popcount;
        pl.scan_grid = dim3(row_blocks, launched_splits);
    }
    if (in.nearby && pl.n_boxes > 0 && (pl.form == HammingForm::MatrixCores || pl.form == HammingForm::Popcount)) {
        pl.box_grid = dim3(row_blocks + launched_splits);
    }
    pl.epilogue_grid = dim3(ceil_div(in.n_ref, kMatchBlock));
    return pl;
}

CosinePlan cosine_plan(const CosinePlanInput &in) {
    CosinePlan pl = {};
    pl.prep_grid = pl.box_grid = pl.recheck_grid = dim3(0);
    pl.dim_pad = (int32_t)align_up((size_t)in.dim, 64);
    pl.margin = pl.dim_pad <= 256 ? kCosineMargin : kCosineMargin + kCosineMarginPerK * (float)(pl.dim_pad - 256);
    // dim <= 256 (SuperPoint, DISK): the ref fragments stay in registers for the whole walk over cur (cosine_gemm_rr_kernel,
    // kRrRows ref rows per workgroup).  Longer descriptors, or FTK_COSINE_CHUNKED=1, use the chunked kernel.
    const bool rs = pl.dim_pad <= 256 && in.chunked != 1;
    const int cur_tile = rs ? kRrTile : kCosineTile, row_group = rs ? kRrRows : kCosineTile;
    pl.n_ref_pad = (int32_t)align_up((size_t)in.n_ref, (size_t)row_group);
    pl.n_cur_pad = (int32_t)align_up((size_t)in.n_cur, (size_t)cur_tile);
    // Keep the whole grid co-resident in ONE round (on-chip ref: one workgroup per CU -> <= 256; chunked: two per
    // CU -> <= 512), each workgroup walking a contiguous run of cur tiles: a second, partly filled round costs more
    // than slightly longer runs.
    const int tiles_total = pl.n_cur_pad / cur_tile;
    int splits = in.splits != kPlanNotSet ? in.splits : (rs ? 256 : 512) / (pl.n_ref_pad / row_group);
    splits = std::max(1, std::min(splits, tiles_total));
    if (rs && in.splits == kPlanNotSet) {
        // At least TWO tiles per split: a walk's first step has no running maximum to cut against yet, so it lists its whole share
        // of every row; with one-tile splits that is all there is, the rows' lists overflow (kCosineCandCap) and the recheck falls
        // back to the exact scan of every pair — 2 000 x 2 000 x 256: 32 splits 17.6 + 3 591 us (contraction + recheck), 16 splits
        // 20.2 + 11.8 us; 1 000 x 1 000 x 128: 16 splits 11.4 + 1 099 us, 8 splits 14.1 + 7.6 us (rocprofv3 kernel trace).
        splits = std::max(1, std::min(splits, tiles_total / 2));
    }
    pl.splits = splits;
    pl.tiles_per_split = ceil_div(tiles_total, splits);
    // the workspace, every region 256-byte aligned
    size_t off = 0;
    auto carve = [&off](size_t bytes) {
        const size_t at = off;
        off += align_up(bytes, 256);
        return at;
    };
    const size_t nr = (size_t)pl.n_ref_pad, nc = (size_t)pl.n_cur_pad;
    pl.ref_h = carve(sizeof(uint16_t) * nr * pl.dim_pad);
    pl.cur_h = carve(sizeof(uint16_t) * nc * pl.dim_pad);
    pl.ref_norm = carve(sizeof(float) * nr);
    pl.cur_norm = carve(sizeof(float) * nc);
    pl.cur_bias = carve(sizeof(float) * nc);
    pl.cur_info = carve(sizeof(float) * 4 * nc);
    pl.tile_box = carve(sizeof(float) * 4 * (nc / kRrTile + 1));
    pl.ref_irregular = carve(nr);
    // row_max | cand_count | irregular_count are adjacent: ONE memset clears them (key 0 = "no candidate yet")
    pl.row_max = carve(sizeof(uint32_t) * nr);
    pl.cand_count = carve(sizeof(uint32_t) * nr);
    pl.irregular_count = carve(sizeof(uint32_t));
    pl.clear_end = off;
    pl.cand = carve(sizeof(int32_t) * nr * kCosineCandCap);
    // the register-stationary kernel walks cur ONCE (running row maximum + scored candidate lists); the chunked kernel runs the
    // maximum-then-collect pair of launches
    pl.ref_stationary = rs ? 1 : 0;
    pl.cand_score = rs ? carve(sizeof(float) * nr * kCosineCandCap) : 0;
    pl.irregular_list = carve(sizeof(int32_t) * kCosineIrregularCap);
    pl.ws_bytes = off;
    // NearbyMatch tile lists (float_matcher_kernels.hip): worth their extra launch from a few thousand candidates on
    pl.use_tile_box = in.nearby && pl.n_cur_pad / kRrTile >= 32;
    // Small calls: ONE exact launch, a wave per ref row (cosine_match_small_kernel); FTK_COSINE_SMALL=0: never
    const bool small = in.small != 0 && (in.dim == 64 || in.dim == 128 || in.dim == 256) && in.n_ref <= kCosineSmallRefMax &&
                       in.n_cur <= (in.nearby ? kCosineSmallCurNearby : kCosineSmallCurForce);
    pl.block = dim3(256);
    if (small) {
        pl.form = CosineForm::Small;
        pl.grid = dim3(ceil_div(in.n_ref, 4));
        return pl;
    }
    pl.packet_prep = in.dim % 8 == 0 && in.aligned16;  // whole 16-byte packets per lane
    const int rows = std::max(pl.n_ref_pad, pl.n_cur_pad);
    pl.prep_grid = dim3(ceil_div((long long)rows * (pl.packet_prep ? 2 : 8), 256), 2);
    if (rs) {
        pl.form = CosineForm::RegisterStationary;
        if (pl.use_tile_box && !pl.packet_prep) {  // (the packet-wide prep kernel writes the boxes itself)
            pl.box_grid = dim3(pl.n_cur_pad / kRrTile);
        }
        pl.grid = dim3((pl.n_ref_pad / kRrRows) * splits);
        pl.block = dim3(512);
        pl.lds = cosine_rr_lds_bytes(pl.dim_pad);
    } else {
        pl.form = CosineForm::Chunked;
        pl.grid = dim3(pl.n_ref_pad / kCosineTile, ceil_div(tiles_total, pl.tiles_per_split));
    }
    pl.recheck_grid = dim3(ceil_div((long long)in.n_ref * 8, 256));
    return pl;
}

DirectPlan direct_plan(const DirectPlanInput &in) {
    DirectPlan pl = {};
    // The per-feature table (an iteration's projections, a level's reference positions and Jacobians) lives in LDS while it fits beside
    // the product ring (64 B per tracked feature, up to kDirectLdsFeatures); larger problems keep that table in device memory instead —
    // same kernel, same arithmetic, same order of the sums.
    pl.feat_in_global = in.max_features > kDirectLdsFeatures;
    pl.feat_bytes = pl.feat_in_global ? align_up(sizeof(float) * 16 * (size_t)in.max_features, 256) : 0;
    pl.poison = in.poison != kPlanNotSet && in.poison != 0;
    // ONE problem (or a handful: a stereo pair, a small rig) with enough terms: spread over the chip (direct_track_spread_kernel) — the
    // one-workgroup kernel is bound by what a single compute unit can issue per iteration.  Exact sums only; FTK_DIRECT_SPREAD=0 keeps
    // the one-workgroup kernel, =n sets the number of producer workgroups per problem (default 32).  Larger batches fill the chip with
    // one workgroup per problem.
    int producers = std::max(0, std::min(in.spread != kPlanNotSet ? in.spread : 32, 200));
    const long long terms = (long long)in.max_features * in.patch_rows * in.patch_cols;
    // below about 256 chunks the producers of one compute unit keep up with the chain (tests spread even tiny problems)
    const long long min_terms = in.min_terms != kPlanNotSet ? in.min_terms : 64ll * 256;
    bool spread = producers > 0 && in.spread_allowed && in.n_problems <= kDirectSpreadMaxProblems && !in.tree && in.method == FTK_METHOD_DIRECT &&
                  !pl.feat_in_global && in.max_features > 0 && terms >= min_terms && terms < (1ll << 31);
    if (spread) {
        // Every workgroup of the launch must be resident at once (consumer and producers wait for each other): size the producers from
        // what THIS device holds — occupancy of the kernel as launched x its compute units (256 on a whole MI355X, 32 on a CPX partition),
        // an eighth left free for whatever else runs — and keep the one-workgroup kernel when fewer than 1 + 2 fit per problem.
        if (in.resident == kPlanNotSet) {
            pl.ask_resident = true;
            return pl;
        }
        const int resident = in.resident_cap != kPlanNotSet ? std::min(in.resident, in.resident_cap) : in.resident;  // (tests: a small partition)
        const int fit = (resident - resident / 8) / in.n_problems - 1;
        producers = std::min(producers, fit);
        // (an explicit FTK_DIRECT_SPREAD=n that fits is honoured: tests)
        spread = producers >= kDirectSpreadMinProducers || (in.spread != kPlanNotSet && producers >= 1 && producers == std::min(in.spread, fit));
    }
    // Workspace: [chunk][7][64] values per problem (the Jacobian row and the residual of every term).  Not beyond 512 MB in total
    // (127 x 127 patches x 768 features would be 347 MB per problem: two such problems keep the one-workgroup kernel), word offsets
    // must fit 32 bits, and a buffer that would have to GROW while the stream is being captured is an error the caller can act on, not
    // a hipMalloc inside the capture: the one-workgroup kernel needs no workspace (same result, capturable).
    const size_t ws = spread ? align_up(direct_spread_ws_bytes(in.max_features, in.patch_rows, in.patch_cols), 256) : 0;
    if (spread && (ws / sizeof(uint32_t) > 0xFFFFFFFFull || ws * (size_t)in.n_problems > (512ull << 20))) {
        spread = false;
    }
    if (spread && ws * (size_t)in.n_problems > in.spread_bytes_held) {
        if (in.capturing == kPlanNotSet) {
            pl.ask_capturing = true;
            return pl;
        }
        spread = !in.capturing;
    }
    if (spread) {
        pl.producers = producers;
        pl.ws_stride = ws;
        pl.clear_bytes = direct_spread_clear_bytes(in.max_features, in.patch_rows, in.patch_cols);
    }
    pl.grid = dim3(spread ? in.n_problems * (1 + producers) : in.n_problems);
    pl.block = dim3(kDmWaves * kWave);
    pl.lds = direct_lds_bytes(pl.feat_in_global ? 0u : in.max_features);
    return pl;
}

// One pass over the matrix, a workgroup per tile of tile_rows x kNnTileCols scores.  The tile is 1 KB wide (a wave's 16-byte loads
// cover a row segment in one instruction) and as tall as leaves about four workgroups for each of the 256 CUs: the pass is a stream
// from HBM / the Infinity Cache, which wants ~32 KB of loads in flight per CU (16 waves x four 1 KB loads), while every tile ends
// with kNnTileCols + tile_rows 8-byte atomics whose number falls with the tile's height.
NnMatchPlan nn_match_plan(const NnMatchPlanInput &in) {
    NnMatchPlan pl = {};
    const long long keys = (long long)in.batch * ((long long)in.n_ref + in.n_cur);
    if (in.batch < 1 || in.n_ref < 1 || in.n_cur < 1 || in.batch > kNnMaxBatch || keys >= (1ll << 31)) {
        return pl;
    }
    pl.vec4 = in.aligned16 && in.row_stride % 4 == 0 && in.batch_stride % 4 == 0;
    pl.col_tiles = ceil_div(in.n_cur, kNnTileCols);
    int rows = kNnTileRowsMax;
    while (rows > kNnTileRowsMin && (long long)in.batch * pl.col_tiles * ceil_div(in.n_ref, rows) < 1024) {
        rows /= 2;
    }
    pl.tile_rows = rows;
    pl.row_tiles = ceil_div(in.n_ref, rows);
    const long long tiles = (long long)pl.row_tiles * pl.col_tiles;
    if (tiles >= (1ll << 31)) {
        return pl;
    }
    pl.ok = true;
    pl.key_count = (size_t)keys + 1;
    pl.grid = dim3((unsigned)tiles, (unsigned)in.batch);
    pl.block = dim3(kNnBlock);
    pl.epilogue_grid = dim3(ceil_div((long long)in.batch * in.n_ref, kNnBlock));
    return pl;
}

}  // namespace ftk
