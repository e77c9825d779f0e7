// transformer_plan_cli — prints the launch plan, workspace layout and packed-weight offsets of the transformer layer
// (csrc/transformer_plan.h) without a device.  One case per line on stdin:
//   rows0 rows1 dim heads aligned16
// one line of key=value pairs per case on stdout.  tests/test_transformer_args_cpu.py drives it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "transformer_plan.h"

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        long long v[5] = {0, 0, 0, 0, 0};
        for (long long &e : v) {
            line >> e;
        }
        const ftk::TransformerPlan p =
            ftk::transformer_plan(ftk::TransformerPlanInput{(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3], (int32_t)v[4]});
        printf("refused=%s", ftk::transformer_refusal_name(p.refused));
        if (p.refused == ftk::TransformerRefusal::None) {
            printf(" head_dim=%d vec_linear=%d vec_attn=%d linear_threads=%d linear_grid_x=%u grid_y_d=%u grid_y_2d=%u grid_y_3d=%u attn_threads=%d"
                   " attn_out_tiles=%d attn_grid_x=%u attn_grid_y=%u attn_grid_z=%u norm_threads=%d norm_blocks=%u launches=%d"
                   " off_qkv=%zu off_ctx=%zu off_msg=%zu off_hidden=%zu off_x1=%zu bytes=%zu weight_floats=%zu",
                   p.head_dim, p.vec_linear, p.vec_attn, 64 * ftk::kLinearWaves, p.linear_grid_x, p.grid_y_d, p.grid_y_2d, p.grid_y_3d,
                   ftk::kAttnThreads, p.attn_out_tiles, p.attn_grid_x, p.attn_grid_y, p.attn_grid_z, ftk::kNormThreads, p.norm_blocks,
                   p.launches, p.qkv.offset, p.ctx.offset, p.msg.offset, p.hidden.offset, p.x1.offset, p.bytes, p.weight_floats);
            for (int k = 0; k < 10; ++k) {
                printf(" w_self%d=%zu w_cross%d=%zu", k, p.w_self[k], k, p.w_cross[k]);
            }
        }
        printf("\n");
    }
    return 0;
}
