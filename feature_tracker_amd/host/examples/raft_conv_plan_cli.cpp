// raft_conv_plan_cli — prints the launch plan of conv2d_kernel (csrc/raft_conv_plan.h) without a device.  One case per line on stdin:
//   out_channels in_channels kernel_size B H W [stride [pool]]
// (a line of six fields is stride 1 and is answered with the fields of stride 1 alone; a seventh adds the strided plan's; an eighth is the
// pool flag of DESIGN.md 5.25 and adds pool=) one line of key=value pairs per case on stdout.  tests/test_update_block_cpu.py drives it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "raft_conv_plan.h"

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        long long v[6] = {0, 0, 0, 0, 0, 0}, stride = 1;
        for (long long &e : v) {
            line >> e;
        }
        long long seventh = 0;
        const bool strided = (bool)(line >> seventh);  // a failed read would store 0
        stride = strided ? seventh : 1;
        long long eighth = 0;
        const bool pooled = strided && (bool)(line >> eighth);
        ftk::ConvPlanInput in{};
        in.out_channels = (int32_t)v[0], in.in_channels = (int32_t)v[1], in.kernel_size = (int32_t)v[2];
        in.B = (int32_t)v[3], in.H = (int32_t)v[4], in.W = (int32_t)v[5];
        in.stride = (int32_t)stride;
        in.pool = pooled ? (int32_t)eighth : 0;
        const ftk::ConvPlan p = ftk::raft_conv_plan(in);
        printf("refused=%s", ftk::conv_refusal_name(p.refused));
        if (p.refused == ftk::ConvRefusal::None) {
            printf(" m_tiles=%d wm=%d wn=%d m_groups=%d tile_w=%d tile_h=%d tiles_x=%d tiles_y=%d chunk=%d chunks=%d steps_per_chunk=%d k_steps=%d"
                   " pitch=%d lds=%zu lds_static=%zu packed=%lld grid=%ux%u block=%ux%u mfma=%s",
                   p.m_tiles, p.wm, p.wn, p.m_groups, p.tile_w, p.tile_h, p.tiles_x, p.tiles_y, p.chunk, p.chunks, p.steps_per_chunk, p.k_steps, p.pitch, p.lds,
                   sizeof(float) * (in.kernel_size == 1 ? ftk::conv_lds_floats(1) : in.kernel_size == 3 ? ftk::conv_lds_floats(3) : ftk::conv_lds_floats(7)),
                   (long long)ftk::raft_conv_packed_elements(in.out_channels, in.in_channels, in.kernel_size), p.grid.x, p.grid.y, p.block.x, p.block.y,
                   p.mfma);
            if (strided) {
                const int ks = in.kernel_size;
                printf(" stride=%d out_h=%d out_w=%d rows=%d row=%d strip_h=%d strip_w=%d lds_static_strided=%zu", p.stride, p.out_h, p.out_w, p.rows, p.row,
                       p.strip_h, p.strip_w,
                       sizeof(float) * (p.stride == 1 ? (ks == 1 ? ftk::conv_lds_floats(1) : ks == 3 ? ftk::conv_lds_floats(3) : ftk::conv_lds_floats(7))
                                                      : (ks == 1 ? ftk::conv_s2_lds_floats(1) : ftk::conv_s2_lds_floats(3))));
            }
            if (pooled) {
                printf(" pool=%d", p.pool);
            }
        }
        printf("\n");
    }
    return 0;
}
