// match_plan_cli — prints the launch plans of the matchers and the direct method (csrc/match_plan.h) without a device.  One case per
// line on stdin, its fields in the order of the plan's input struct, "-" for an override or input that is not set (kPlanNotSet):
//   hamming n_ref n_cur n_words n_bits nearby keys_given small kernel
//   cosine  n_ref n_cur dim nearby aligned16 small chunked splits
//   direct  n_problems max_features patch_rows patch_cols method tree spread_allowed resident capturing held spread resident_cap poison min_terms
//   nn      batch n_ref n_cur row_stride batch_stride aligned16
// one line of key=value pairs per case on stdout.  tests/test_match_plan_cpu.py drives it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "match_plan.h"

static long long field(std::istringstream &line) {
    std::string w;
    line >> w;
    return w == "-" ? ftk::kPlanNotSet : atoll(w.c_str());
}

static void grid(const char *name, const dim3 &d) { printf(" %s=%ux%u", name, d.x, d.y); }

int main() {
    static const char *const hamming_forms[] = {"small", "plain", "popcount", "matrix_cores", "generic"};
    static const char *const cosine_forms[] = {"small", "register_stationary", "chunked"};
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        std::string kind;
        line >> kind;
        if (kind == "hamming") {
            ftk::HammingPlanInput in;
            in.n_ref = (int32_t)field(line), in.n_cur = (int32_t)field(line), in.n_words = (int32_t)field(line), in.n_bits = (int32_t)field(line);
            in.nearby = (int)field(line), in.keys_given = (int)field(line), in.small = (int)field(line), in.kernel = (int)field(line);
            const ftk::HammingPlan p = ftk::hamming_plan(in);
            printf("form=%s dev_words=%d pad=%d cur_per_block=%d keys_clean=%d matrix_cores=%d n_boxes=%zu", hamming_forms[(int)p.form], p.dev_words, p.dev_words != in.n_words,
                   p.cur_per_block, p.keys_clean, p.matrix_cores, p.n_boxes);
            grid("box_grid", p.box_grid), grid("scan_grid", p.scan_grid), grid("scan_block", p.scan_block), grid("epilogue_grid", p.epilogue_grid);
        } else if (kind == "cosine") {
            ftk::CosinePlanInput in;
            in.n_ref = (int32_t)field(line), in.n_cur = (int32_t)field(line), in.dim = (int32_t)field(line), in.nearby = (int)field(line);
            in.aligned16 = (int)field(line), in.small = (int)field(line), in.chunked = (int)field(line), in.splits = (int)field(line);
            const ftk::CosinePlan p = ftk::cosine_plan(in);
            printf("form=%s dim_pad=%d n_ref_pad=%d n_cur_pad=%d splits=%d tiles_per_split=%d ref_stationary=%d use_tile_box=%d packet_prep=%d lds=%zu",
                   cosine_forms[(int)p.form], p.dim_pad, p.n_ref_pad, p.n_cur_pad, p.splits, p.tiles_per_split, p.ref_stationary, p.use_tile_box, p.packet_prep, p.lds);
            printf(" ref_h=%zu cur_h=%zu ref_norm=%zu cur_norm=%zu cur_bias=%zu cur_info=%zu tile_box=%zu ref_irregular=%zu row_max=%zu cand_count=%zu"
                   " irregular_count=%zu clear_end=%zu cand=%zu cand_score=%zu irregular_list=%zu ws_bytes=%zu",
                   p.ref_h, p.cur_h, p.ref_norm, p.cur_norm, p.cur_bias, p.cur_info, p.tile_box, p.ref_irregular, p.row_max, p.cand_count, p.irregular_count,
                   p.clear_end, p.cand, p.cand_score, p.irregular_list, p.ws_bytes);
            printf(" margin=%.9g", (double)p.margin);
            grid("prep_grid", p.prep_grid), grid("box_grid", p.box_grid), grid("grid", p.grid), grid("block", p.block), grid("recheck_grid", p.recheck_grid);
        } else if (kind == "direct") {
            ftk::DirectPlanInput in;
            in.n_problems = (int32_t)field(line), in.max_features = (uint32_t)field(line), in.patch_rows = (int32_t)field(line);
            in.patch_cols = (int32_t)field(line), in.method = (int)field(line), in.tree = (int)field(line), in.spread_allowed = (int)field(line);
            in.resident = (int)field(line), in.capturing = (int)field(line), in.spread_bytes_held = (size_t)field(line), in.spread = (int)field(line);
            in.resident_cap = (int)field(line), in.poison = (int)field(line), in.min_terms = field(line);
            const ftk::DirectPlan p = ftk::direct_plan(in);
            printf("ask_resident=%d ask_capturing=%d feat_in_global=%d feat_bytes=%zu producers=%d ws_stride=%zu clear_bytes=%zu poison=%d lds=%zu", p.ask_resident,
                   p.ask_capturing, p.feat_in_global, p.feat_bytes, p.producers, p.ws_stride, p.clear_bytes, p.poison, p.lds);
            grid("grid", p.grid), grid("block", p.block);
        } else if (kind == "nn") {
            ftk::NnMatchPlanInput in;
            in.batch = (int32_t)field(line), in.n_ref = (int32_t)field(line), in.n_cur = (int32_t)field(line);
            in.row_stride = field(line), in.batch_stride = field(line), in.aligned16 = (int)field(line);
            const ftk::NnMatchPlan p = ftk::nn_match_plan(in);
            printf("ok=%d vec4=%d tile_rows=%d tile_cols=%d row_tiles=%d col_tiles=%d key_count=%zu", p.ok, p.vec4, p.tile_rows, ftk::kNnTileCols, p.row_tiles,
                   p.col_tiles, p.key_count);
            grid("grid", p.grid), grid("block", p.block), grid("epilogue_grid", p.epilogue_grid);
        } else {
            printf("error=unknown_kind");
        }
        printf("\n");
    }
    return 0;
}
